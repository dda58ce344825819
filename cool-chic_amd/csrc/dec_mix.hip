// dec_mix.hip -- path B: the mix stage of the decoder's output stage (ccmi_mix, steps 4, 4e, 4m, 5 and 6
// of the contract in ccmi.h): RandomErasing, MixUp and CutMix on the normalised frame, before the one
// rounding to the element type.
//
// The mix-staged frames of a call leave their tails in float32 in the workspace (the filter stage's
// staging frame, or the filter kernel's float32 output where it had a blur or a solarize to compute).
//
//  dec_mix_batch<T>   one launch per call, after every chunk and tail group has been joined (a partner may
//                     sit in any of them): reads the frame and, with a partner, the partner's frame,
//                     and writes the caller's tensor in the call's format (fmt_group_at / fmt_store of
//                     dec_out_fmt.h).  blockIdx.y is the frame's entry of the mix table.
//
// Element type, scale and bias are the call's; size and resolved strides are each frame's own and come
// from its entry (all-zero strides resolve to every frame's own size), so the grid covers the call's
// largest mix-staged frame and a block outside its frame leaves at once.
// A block owns a tile of kTileH rows x kTileG groups of 4 destination pixels, one group per thread.  The
// entry, and the partner's, come in by scalar loads (blockIdx.y and the partner's index are uniform);
// whether the tile meets any rectangle, any noise rectangle or the box is decided once per block from
// those scalars, so a tile away from every rectangle runs step 4, the blend and the store only, and only a
// tile that meets a rectangle with sigma > 0 pays for the draws (two mix64, logf, sqrtf, cospif per
// element).  A stream: 12 (24 with a partner) bytes read and 3 sizeof(T) written per pixel, no LDS.
// Every product and sum is its own float32 operation (fmt_mul / fmt_add), in the contract's order.
#include "dec_mix_entry.h"

namespace ccmi {
namespace {

// steps 4 and 4e of frame E for the thread's 4 pixels d0 .. d0 + 3 of row y: a[c][k]
__device__ __forceinline__ void staged_group(const DecMixEntry &E, const DecFmtCall &C, bool live, int y, int d0, bool any,
                                             bool noisy, float (&a)[3][4])
{
    const int oh = E.oh, ow = E.ow;
    const unsigned plane = (unsigned)oh * (unsigned)ow; // 3 oh ow <= 3 * 2^28: 32-bit element offsets
    // the pointer comes out of the table: say that it is global memory, or every load is a flat one
    const GlobalFloat *__restrict__ src = (const GlobalFloat *)E.src;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned at = c * plane + (unsigned)y * (unsigned)ow;
#pragma unroll
        for (int k = 0; k < 4; ++k) { // the surplus slots of a partial group are never stored
            const float v = live ? src[at + (unsigned)min(max(d0 + k, 0), ow - 1)] : 0.f;
            a[c][k] = fmt_add(fmt_mul(v, C.scale[c]), C.bias[c]);
        }
    }
    if (!any) return; // uniform: the tile meets none of the frame's rectangles
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

template <typename T>
__global__ __launch_bounds__(kThreads) void dec_mix_batch(const DecMixEntry *__restrict__ Es, int first, DecFmtCall C,
                                                          int tiles_x)
{
    const DecMixEntry &E = Es[first + (int)blockIdx.y]; // a partner's entry counts from the table's start
    C.sc = E.sc, C.sy = E.sy, C.sx = E.sx;              // scale and bias are the call's, the strides the frame's
    const int oh = E.oh, ow = E.ow;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * kTileH, g0 = tx * kTileG;
    if (y0 >= oh || g0 >= fmt_row_groups(ow)) return; // the grid covers the call's largest frame
    // the pixels the tile's groups can touch: up to 3 lead-in slots before 4 g0
    const int x0 = 4 * g0 - 3, x1 = 4 * (g0 + kTileG), y1 = y0 + kTileH;

    const int tid = threadIdx.x;
    const int y = y0 + tid / kTileG;
    T *__restrict__ dst = static_cast<T *>(E.dst); // fmt_store takes a generic pointer: its stores stay flat ones
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
    staged_group(E, C, live, y, d0, any, noisy, a);

    if (E.partner >= 0) {
        const DecMixEntry &P = Es[E.partner];
        const bool boxed = E.bw > 0;
        // CutMix away from the box: the partner does not enter
        if (!boxed || meets(x0, x1, y0, y1, E.bx, E.by, E.bw, E.bh)) {
            bool pany = false, pnoisy = false;
            for (int t = 0; t < P.count; ++t) {
                const bool hit = meets(x0, x1, y0, y1, P.r[t].x, P.r[t].y, P.r[t].w, P.r[t].h);
                pany = pany || hit, pnoisy = pnoisy || (hit && P.r[t].sigma > 0.f);
            }
            float b[3][4];
            staged_group(P, C, live, y, d0, pany, pnoisy, b);
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

void dec_mix_fill(void *host_tab, const DecTailFrame &f, int oh, int ow, int partner_entry)
{
    const DecMix &m = *f.mix;
    DecMixEntry e{};
    e.src = dec_mix_source(f);
    e.dst = f.dst;
    e.seed = m.seed;
    e.oh = oh, e.ow = ow;
    e.partner = partner_entry;
    e.count = m.count;
    e.lam = m.lam, e.oml = m.oml;
    e.bx = m.box[0], e.by = m.box[1], e.bw = m.box[2], e.bh = m.box[3];
    for (int t = 0; t < CCMI_MIX_MAX_RECTS; ++t) e.r[t] = m.r[t];
    e.sc = f.fmt.stride_c, e.sy = f.fmt.stride_y, e.sx = f.fmt.stride_x;
    static_cast<DecMixEntry *>(host_tab)[m.entry] = e;
}

int launch_dec_mix(const void *dev_tab, int n_entries, int max_oh, int max_ow, const DecFmt &fmt, hipStream_t s)
{
    if (n_entries < 1 || max_oh < 1 || max_ow < 1 || !fmt.on) return ccmi_set_error(CCMI_ERR_ARG, "dec: mix launch of %d frames", n_entries);
    const DecMixEntry *es = static_cast<const DecMixEntry *>(dev_tab);
    const int tiles_x = mix_tiles_x(max_ow);
    const DecFmtCall C = fmt_call(fmt);
    for (int first = 0; first < n_entries; first += 65535) {
        const int m = n_entries - first < 65535 ? n_entries - first : 65535;
        const dim3 grid((unsigned)(tiles_x * mix_tiles_y(max_oh)), (unsigned)m);
        if (int rc = with_elem_type(fmt.elem, [&](auto t) {
                hipLaunchKernelGGL(dec_mix_batch<decltype(t)>, grid, dim3(kThreads), 0, s, es, first, C, tiles_x);
            }))
            return rc;
    }
    return CCMI_OK;
}

} // namespace ccmi
