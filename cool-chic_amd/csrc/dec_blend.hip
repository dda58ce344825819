// dec_blend.hip -- path B: the blend stage of the decoder's output stage (ccmi_blend, step 3b of the contract
// in ccmi.h): weighted sums of up to CCMI_BLEND_MAX_TERMS staged frames of the call before the normalisation,
// and silent frames that are sources only -- what AugMix needs.
//
//  dec_blend_batch<T> the call's one launch after the join, in place of dec_mix_batch, for a call with a
//                     ccmi_blend: the form of dec_mix_batch whose frame, and whose partner, is a weighted sum
//                     of K staged frames of the call.  The number of terms sits in the frame's mix entry, the
//                     sources' entries and the weights in its entry of the blend table (the mix table's
//                     sibling); all of it, and the sources' entries, come in by scalar loads and the loop
//                     over the terms is uniform.  An entry without a destination (a silent frame: a source
//                     only) leaves at block start.  12 K bytes read per pixel (12 K_p more where the partner
//                     enters), 3 sizeof(T) written, no LDS.
// The tile, the entry and steps 4, 4e, 4m, 5 and 6 are the mix stage's (dec_mix.hip, dec_mix_entry.h).
#include "dec_mix_entry.h"

namespace ccmi {
namespace {

// the terms of one mix-staged frame: kBlendTableBytes of the call's blend table
struct DecBlendEntry {
    int src[CCMI_BLEND_MAX_TERMS]; // the sources' entries of the mix table
    float w[CCMI_BLEND_MAX_TERMS];
};
static_assert(sizeof(DecBlendEntry) == kBlendTableBytes, "the blend entry of kBlendTableBytes");

// step 4e of frame E on a[c][k], for a tile that meets one of its rectangles (staged_group of dec_mix.hip
// has the step in its own body)
__device__ __forceinline__ void erase_group(const DecMixEntry &E, unsigned plane, int y, int d0, bool noisy, float (&a)[3][4])
{
    const int ow = E.ow;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the last rectangle that holds the pixel wins: its value and sigma
        const int x = d0 + k;
        bool hit = false;
        float ev[3] = {0.f, 0.f, 0.f}, es = 0.f;
        for (int t = 0; t < E.count; ++t) {
            const DecMixRect &R = E.r[t];
            if (y >= R.y && y < R.y + R.h && x >= R.x && x < R.x + R.w) hit = true, ev[0] = R.v[0], ev[1] = R.v[1], ev[2] = R.v[2], es = R.sigma;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float e = ev[c];
            if (noisy) { // uniform: the tile meets a rectangle with sigma > 0
                const unsigned index = c * plane + (unsigned)y * (unsigned)ow + (unsigned)x;
                const float g = fmt_mul(gauss_unit(mix64(E.seed ^ mix64((uint64_t)index))), es);
                e = es == 0.f ? e : fmt_add(e, g);
            }
            a[c][k] = hit ? e : a[c][k];
        }
    }
}

// steps 3b, 4 and 4e of entry e for the thread's 4 pixels: staged_group with the frame's terms in place of
// the frame.  Every source has the frame's size (the plan's check), so one offset serves them all.
__device__ __forceinline__ void blended_group(const DecMixEntry *__restrict__ Es, const DecBlendEntry *__restrict__ Bs, int e,
                                              const DecFmtCall &C, bool live, int y, int d0, bool any, bool noisy,
                                              float (&a)[3][4])
{
    const DecMixEntry &E = Es[e];
    const DecBlendEntry &B = Bs[e];
    const int ow = E.ow, K = E.terms;
    const unsigned plane = (unsigned)E.oh * (unsigned)ow;
    unsigned at[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) at[k] = (unsigned)y * (unsigned)ow + (unsigned)min(max(d0 + k, 0), ow - 1);
    // a channel at a time: 4 loads of a term in flight beside the 12 sums (and the 12 of the frame while the
    // partner is summed), which keeps the kernel at 8 waves per SIMD
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned base = c * plane;
        {
            const GlobalFloat *__restrict__ src = (const GlobalFloat *)(K > 0 ? Es[B.src[0]].src : E.src);
            const float w = B.w[0];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = live ? src[base + at[k]] : 0.f;
                a[c][k] = K > 0 ? fmt_mul(w, v) : v;
            }
        }
        for (int t = 1; t < K; ++t) { // uniform: K is the entry's
            const GlobalFloat *__restrict__ src = (const GlobalFloat *)Es[B.src[t]].src;
            const float w = B.w[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[c][k] = fmt_add(a[c][k], fmt_mul(w, live ? src[base + at[k]] : 0.f));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[c][k] = fmt_add(fmt_mul(a[c][k], C.scale[c]), C.bias[c]);
    }
    if (any) erase_group(E, plane, y, d0, noisy, a);
}

// 8 waves per SIMD asked for: the frame's 12 sums, the partner's 12 and a term's loads fit 64 VGPRs
template <typename T>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8))) void dec_blend_batch(
    const DecMixEntry *__restrict__ Es, const DecBlendEntry *__restrict__ Bs, int first, DecFmtCall C, int tiles_x)
{
    const int e = first + (int)blockIdx.y;
    const DecMixEntry &E = Es[e];
    if (!E.dst) return; // a silent frame: a source only
    C.sc = E.sc, C.sy = E.sy, C.sx = E.sx;
    const int oh = E.oh, ow = E.ow;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTileH, g0 = tx * kTileG;
    if (y0 >= oh || g0 >= fmt_row_groups(ow)) return;
    const int x0 = 4 * g0 - 3, x1 = 4 * (g0 + kTileG), y1 = y0 + kTileH;

    const int tid = threadIdx.x;
    const int y = y0 + tid / kTileG;
    T *__restrict__ dst = static_cast<T *>(E.dst);
    int d0 = 0;
    int64_t row = 0;
    bool nchw = false, nhwc = false;
    const bool live = y < oh && fmt_group_at<T>(dst, C, y, g0 + (tid & (kTileG - 1)), ow, d0, row, nchw, nhwc);

    bool any = false, noisy = false;
    for (int t = 0; t < E.count; ++t) {
        const bool hit = meets(x0, x1, y0, y1, E.r[t].x, E.r[t].y, E.r[t].w, E.r[t].h);
        any = any || hit, noisy = noisy || (hit && E.r[t].sigma > 0.f);
    }
    float a[3][4];
    blended_group(Es, Bs, e, C, live, y, d0, any, noisy, a);

    if (E.partner >= 0) {
        const DecMixEntry &P = Es[E.partner];
        const bool boxed = E.bw > 0;
        if (!boxed || meets(x0, x1, y0, y1, E.bx, E.by, E.bw, E.bh)) {
            bool pany = false, pnoisy = false;
            for (int t = 0; t < P.count; ++t) {
                const bool hit = meets(x0, x1, y0, y1, P.r[t].x, P.r[t].y, P.r[t].w, P.r[t].h);
                pany = pany || hit, pnoisy = pnoisy || (hit && P.r[t].sigma > 0.f);
            }
            float b[3][4];
            blended_group(Es, Bs, E.partner, C, live, y, d0, pany, pnoisy, b); // the partner with its own step 3b
            const bool row_in = y >= E.by && y < E.by + E.bh;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = d0 + k;
                const bool in = row_in && x >= E.bx && x < E.bx + E.bw;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    a[c][k] = boxed ? (in ? b[c][k] : a[c][k]) : fmt_add(fmt_mul(E.lam, a[c][k]), fmt_mul(E.oml, b[c][k]));
            }
        }
    }
    if (!live) return;
    T v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = fmt_elem<T>(a[c][k]);
    fmt_store<T>(v, dst, C, row, d0, ow, nchw, nhwc);
}

} // namespace

void dec_blend_fill(void *host_mix_tab, void *host_blend_tab, int entry, const DecBlend &b, const int *src_entries)
{
    DecMixEntry &e = static_cast<DecMixEntry *>(host_mix_tab)[entry];
    e.terms = b.count;
    if (b.silent) e.dst = nullptr;
    DecBlendEntry &t = static_cast<DecBlendEntry *>(host_blend_tab)[entry];
    for (int k = 0; k < b.count; ++k) t.src[k] = src_entries[k], t.w[k] = b.w[k];
}

int launch_dec_blend(const void *dev_mix_tab, const void *dev_blend_tab, int n_entries, int max_oh, int max_ow,
                     const DecFmt &fmt, hipStream_t s)
{
    if (n_entries < 1 || max_oh < 1 || max_ow < 1 || !fmt.on) return ccmi_set_error(CCMI_ERR_ARG, "dec: blend launch of %d frames", n_entries);
    const DecMixEntry *es = static_cast<const DecMixEntry *>(dev_mix_tab);
    const DecBlendEntry *bs = static_cast<const DecBlendEntry *>(dev_blend_tab);
    const int tiles_x = mix_tiles_x(max_ow);
    const DecFmtCall C = fmt_call(fmt);
    for (int first = 0; first < n_entries; first += 65535) {
        const int m = n_entries - first < 65535 ? n_entries - first : 65535;
        const dim3 grid((unsigned)(tiles_x * mix_tiles_y(max_oh)), (unsigned)m);
        if (int rc = with_elem_type(fmt.elem, [&](auto t) {
                hipLaunchKernelGGL(dec_blend_batch<decltype(t)>, grid, dim3(kThreads), 0, s, es, bs, first, C, tiles_x);
            }))
            return rc;
    }
    return CCMI_OK;
}

} // namespace ccmi
