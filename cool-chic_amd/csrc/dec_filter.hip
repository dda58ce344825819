// dec_filter.hip -- path B: the filter stage of the decoder's output stage (ccmi_filter, steps 3y-0
// to 3y-2 of the contract in ccmi.h): a per-frame separable blur with reflecting borders and a
// per-frame solarize, between the colour ops and scale / bias.
//
// Blur is the one operation of the output stage that needs a pixel's neighbours AFTER the geometry
// and the colour ops, so the frames that take the stage are staged: the group's own geometry and
// colour kernels (dec_out.hip, unchanged) run once more over them in the identity format -- float32,
// planar, scale 1, bias 0, the frame's mirror -- into one float32 frame [3][oh][ow] each; the tone ops
// of a call with a ccmi_tone (dec_tone.hip) then run on the staged frames, in place or into a frame's
// second buffer; and
//
//  dec_filter<T>, dec_filter_batch<T>   read those frames and write the caller's tensors in the
//                   call's format (steps 4-6: fmt_group_at / fmt_store of dec_out_fmt.h), one launch
//                   for both passes and for frames of any radii, 0 (solarize only) included.
//
// A block owns a tile of kTileH rows x kTileG groups of 4 destination pixels of one frame.  The groups
// of a row start up to 3 pixels before a multiple of 4 (the row's alignment, fmt_group_at), so the
// tile spans kTileW = 4 kTileG + 3 columns.  Per channel the block loads the tile and its r-wide halo
// into LDS through two index tables (refl() once per halo row and column, not per element), runs the
// horizontal pass over the tile's rows and the vertical halo into a second LDS array -- the
// horizontal result never goes to memory; the halo rows are computed again by the tile above and
// below -- and the vertical pass into registers, where solarize and steps 4-5 follow; after the third
// channel the thread stores its groups.  The radius is one per block: the loop bounds are scalars and
// the taps come from the frame's table entry by scalar loads.
// Every product and sum is its own float32 operation (fmt_mul / fmt_add), in the contract's order.
#include <string.h>

#include "dec_out_fmt.h"

namespace ccmi {
namespace {

constexpr int kThreads = kOutThreads;
constexpr int kR = CCMI_FLT_MAX_RADIUS;
constexpr int kTileH = 32;              // rows of a tile: two per thread
constexpr int kTileG = 16;              // groups of 4 destination pixels per tile row
constexpr int kTileW = 4 * kTileG + 3;  // columns a tile's groups can touch
constexpr int kInH = kTileH + 2 * kR, kInW = kTileW + 2 * kR; // the tile with its halo
// pitch of the horizontal result: 5 mod 32, so the rows a wave reads in the vertical pass (lanes
// 4 columns apart within a row) start on different banks
constexpr int kHPitch = 69;
static_assert(kThreads == 16 * kTileG && kTileH == 2 * (kThreads / kTileG), "a thread owns group gi of rows ly and ly + 16");
static_assert(kInW <= 128, "the load walks a halo row with 128 threads");

// one staged frame: where it is staged, where it goes, and its filter (DecFlt)
struct DecFltEntry {
    const float *src; // [3][oh][ow], the frame as it will be stored (mirrored already), before step 4
    void *dst;
    int r, sol;
    float th;
    int pad_;
    float taps[kR + 1];
};
static_assert(sizeof(DecFltEntry) == 96, "the filter entry of kFltTableBytes");

// refl(a, n) of the contract: reflection without repeating the border, folded as often as needed
__device__ __forceinline__ int flt_refl(int a, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = a % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

template <typename T>
__device__ __forceinline__ void filter_body(const DecFltEntry &F, int oh, int ow, const DecFmtCall &C, int tiles_x)
{
    __shared__ float s_in[kInH * kInW];   // one channel of the tile and its halo
    __shared__ float s_h[kInH * kHPitch]; // its horizontal pass, tile columns only
    __shared__ int s_row[kInH], s_col[kInW]; // element offsets of the halo's rows and columns in a plane
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y_base = ty * kTileH, x_base = tx * 4 * kTileG - 3;
    const int r = F.r;
    const int in_h = min(kTileH, oh - y_base) + 2 * r, in_w = kTileW + 2 * r;
    const unsigned plane = (unsigned)oh * (unsigned)ow; // 3 oh ow <= 3 * 2^28: 32-bit element offsets
    const float *__restrict__ src = F.src;
    T *__restrict__ dst = static_cast<T *>(F.dst);

    // the thread's two groups: group gi of tile rows ly0 and ly0 + 16
    const int gi = tid & (kTileG - 1), ly0 = tid / kTileG;
    bool live[2], nchw = false, nhwc = false;
    int d0[2], lk[2];
    int64_t row[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int y = y_base + ly0 + 16 * j;
        d0[j] = 0, row[j] = 0;
        live[j] = y < oh && fmt_group_at<T>(dst, C, y, tx * kTileG + gi, ow, d0[j], row[j], nchw, nhwc);
        lk[j] = live[j] ? d0[j] - x_base : 0; // 4 gi + 3 - mis: 0 .. kTileW - 4
    }
    if (r > 0) {
        for (int i = tid; i < in_h; i += kThreads) s_row[i] = flt_refl(y_base - r + i, oh) * ow;
        for (int i = tid; i < in_w; i += kThreads) s_col[i] = flt_refl(x_base - r + i, ow);
    }
    T v[2][3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc[2][4];
        if (r > 0) {
            __syncthreads(); // the index tables are written; the channel before is read
            for (int ly = tid >> 7; ly < in_h; ly += kThreads >> 7) {
                const int lx = tid & 127;
                if (lx < in_w) s_in[ly * kInW + lx] = src[c * plane + (unsigned)(s_row[ly] + s_col[lx])];
            }
            __syncthreads();
            for (int idx = tid; idx < in_h * kTileW; idx += kThreads) {
                const int ly = idx / kTileW, k = idx - ly * kTileW;
                const float *__restrict__ p = s_in + ly * kInW + k + r;
                float t = 0.f;
                for (int d = -r; d <= r; ++d) t = fmt_add(t, fmt_mul(F.taps[d < 0 ? -d : d], p[d]));
                s_h[ly * kHPitch + k] = t;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j][k] = 0.f;
            for (int d = -r; d <= r; ++d) {
                const float w = F.taps[d < 0 ? -d : d];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float *__restrict__ p = s_h + (ly0 + 16 * j + r + d) * kHPitch + lk[j];
                    if (live[j]) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[j][k] = fmt_add(acc[j][k], fmt_mul(w, p[k]));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j][k] = fminf(fmaxf(acc[j][k], 0.f), 1.f);
        } else { // solarize only: y = x
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned at = c * plane + (unsigned)(y_base + ly0 + 16 * j) * (unsigned)ow;
#pragma unroll
                for (int k = 0; k < 4; ++k) // the surplus slots of a partial group are never stored
                    acc[j][k] = live[j] ? src[at + (unsigned)min(max(d0[j] + k, 0), ow - 1)] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float y = acc[j][k];
                if (F.sol) y = y >= F.th ? 1.0f - y : y;
                v[j][c][k] = fmt_elem<T>(fmt_add(fmt_mul(y, C.scale[c]), C.bias[c]));
            }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (live[j]) fmt_store<T>(v[j], dst, C, row[j], d0[j], ow, nchw, nhwc);
}

// one frame (the per-frame tail)
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_filter(DecFltEntry F, int oh, int ow, DecFmtCall C, int tiles_x)
{
    filter_body<T>(F, oh, ow, C, tiles_x);
}

// the staged frames of a tail group: frame blockIdx.y's entry
template <typename T>
__global__ __launch_bounds__(kThreads) void dec_filter_batch(const DecFltEntry *__restrict__ Fs, int oh, int ow, DecFmtCall C,
                                                             int tiles_x)
{
    filter_body<T>(Fs[blockIdx.y], oh, ow, C, tiles_x);
}

int filter_tiles_x(int ow) { return (fmt_row_groups(ow) + kTileG - 1) / kTileG; }
int filter_tiles_y(int oh) { return (oh + kTileH - 1) / kTileH; }

DecFltEntry filter_entry(const DecTailFrame &f)
{
    DecFltEntry e{};
    // a frame's tone ops leave it in its second buffer after an odd number of sharpness passes
    e.src = f.tone ? f.tone->buf[dec_tone_sharps(*f.tone) & 1] : f.flt_tmp;
    e.dst = f.mix ? static_cast<void *>(f.mix_buf) : f.dst; // a mix-staged frame stays in float32 (identity_call)
    e.r = f.flt->r, e.sol = f.flt->sol, e.th = f.flt->th;
    memcpy(e.taps, f.flt->taps, sizeof e.taps);
    return e;
}

// the size of the frame a formatted sink stores, from its h x w synthesis region
void stored_size(const DecFmt &fmt, int h, int w, int &oh, int &ow)
{
    const bool sized = fmt.rs || fmt.warp;
    oh = sized ? fmt.out_h : h, ow = sized ? fmt.out_w : w;
}

// f as the staging launch sees it: the same geometry, mirror and colour ops in the identity format
// (float32, planar, scale 1, bias 0: q 1 + 0 is q with a -0 turned into +0, exactly) into the staging frame
DecTailFrame staged_frame(const DecTailFrame &f, int oh, int ow)
{
    DecTailFrame t = f;
    t.dst = reinterpret_cast<uint8_t *>(f.flt_tmp);
    t.fmt.elem = CCMI_ELEM_F32;
    for (int c = 0; c < 3; ++c) t.fmt.scale[c] = 1.f, t.fmt.bias[c] = 0.f;
    t.fmt.stride_c = (int64_t)oh * ow, t.fmt.stride_y = ow, t.fmt.stride_x = 1;
    t.flt = nullptr;
    return t;
}

// the identity format as the filter kernel's own launch argument: what it writes for a mix-staged frame,
// [3][oh][ow] float32 at DecTailFrame::mix_buf (y 1 + 0: y with a -0 turned into +0)
DecFmtCall identity_call(int oh, int ow)
{
    DecFmtCall C;
    for (int c = 0; c < 3; ++c) C.scale[c] = 1.f, C.bias[c] = 0.f;
    C.sc = (int64_t)oh * ow, C.sy = ow, C.sx = 1;
    return C;
}

size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// the filter entries of a group of m staged frames follow their staging entries
size_t filter_entries_off(const DecFmt &fmt, int m) { return al16(dec_out_entry_bytes(dec_out_form(fmt)) * (size_t)m); }

int check_staged(const DecTailFrame &f)
{
    if (!f.fmt.on || !f.flt || !f.flt_tmp || !f.dst) return ccmi_set_error(CCMI_ERR_ARG, "dec: a filter without its staging frame");
    if (f.flt->r < 0 || f.flt->r > kR) return ccmi_set_error(CCMI_ERR_ARG, "dec: filter radius %d", f.flt->r);
    if (dec_flt_class(f) == 1 && !f.mix_buf) return ccmi_set_error(CCMI_ERR_ARG, "dec: a mix-staged frame without its second frame");
    return CCMI_OK;
}

} // namespace

const float *dec_mix_source(const DecTailFrame &f) { return dec_flt_class(f) == 1 ? f.mix_buf : filter_entry(f).src; }

void dec_flt_fill(void *flt_tab, int m, int i, const DecTailFrame &f, int h, int w, int oy, int ox)
{
    int oh, ow;
    stored_size(f.fmt, h, w, oh, ow);
    DecTailFrame t = staged_frame(f, oh, ow);
    t.fmt.col = 0; // the group's colour section holds the frame's ops already
    dec_out_fill(flt_tab, nullptr, i, t, h, w, oy, ox);
    DecFltEntry *fe = reinterpret_cast<DecFltEntry *>(static_cast<uint8_t *>(flt_tab) + filter_entries_off(f.fmt, m));
    fe[i] = filter_entry(f);
    if (f.tone) reinterpret_cast<DecTone *>(static_cast<uint8_t *>(flt_tab) + kFltTableBytes * (size_t)m)[i] = *f.tone;
}

int launch_dec_out_group_flt(const DecTailFrame *const *fr, int m, int h, int w, const void *dev_flt_tab,
                             const DecCol *col_sec, hipStream_t s)
{
    const DecTailFrame &f0 = *fr[0];
    bool stat = false;
    for (int i = 0; i < m; ++i) {
        if (int rc = check_staged(*fr[i])) return rc;
        stat = stat || (fr[i]->fmt.col && fr[i]->col->contrast >= 0);
    }
    // one stored size per group: a region group has one region size, a sized one its output size
    int oh, ow;
    stored_size(f0.fmt, h, w, oh, ow);
    if (int rc = launch_dec_out_group(staged_frame(f0, oh, ow), h, w, m, dev_flt_tab, col_sec, stat, s)) return rc;
    const DecFltEntry *fe =
        reinterpret_cast<const DecFltEntry *>(static_cast<const uint8_t *>(dev_flt_tab) + filter_entries_off(f0.fmt, m));
    if (f0.tone) { // the tone ops of the staged frames, segment after segment, on the staging frames
        std::vector<const DecTone *> es(m);
        for (int i = 0; i < m; ++i) {
            if (!fr[i]->tone) return ccmi_set_error(CCMI_ERR_ARG, "dec: a staged frame without its tone entry");
            es[i] = fr[i]->tone;
        }
        const DecTone *dev_es =
            reinterpret_cast<const DecTone *>(static_cast<const uint8_t *>(dev_flt_tab) + kFltTableBytes * (size_t)m);
        if (int rc = launch_dec_tone_group(dev_es, es.data(), m, oh, ow, s)) return rc;
    }
    // the frames the filter kernel formats, then the mix-staged ones it filters in float32, then the
    // mix-staged ones it has nothing to do for (dec_flt_class: 0, 1, 2, in this order)
    int m0 = 0, m1 = 0;
    for (int i = 0; i < m; ++i) {
        const int k = dec_flt_class(*fr[i]);
        if (k < (i ? dec_flt_class(*fr[i - 1]) : 0)) return ccmi_set_error(CCMI_ERR_ARG, "dec: staged frames out of order");
        m0 += k == 0, m1 += k == 1;
    }
    const int tiles_x = filter_tiles_x(ow);
    if (m0 > 0) {
        const dim3 grid((unsigned)(tiles_x * filter_tiles_y(oh)), (unsigned)m0);
        const DecFmtCall C = fmt_call(f0.fmt);
        if (int rc = with_elem_type(f0.fmt.elem, [&](auto t) {
                hipLaunchKernelGGL(dec_filter_batch<decltype(t)>, grid, dim3(kThreads), 0, s, fe, oh, ow, C, tiles_x);
            }))
            return rc;
    }
    if (m1 > 0) {
        const dim3 grid((unsigned)(tiles_x * filter_tiles_y(oh)), (unsigned)m1);
        hipLaunchKernelGGL(dec_filter_batch<float>, grid, dim3(kThreads), 0, s, fe + m0, oh, ow, identity_call(oh, ow), tiles_x);
        CCMI_HIP_CHECK(hipGetLastError());
    }
    return CCMI_OK;
}

int launch_dec_out_frame_flt(const DecTailFrame &f, const int32_t *synout, int h, int w, hipStream_t s)
{
    if (int rc = check_staged(f)) return rc;
    // the stored frame: the region f.roi.rect of the whole-frame synthesis output, or the output size
    int oh, ow;
    stored_size(f.fmt, f.roi.rect.h(), f.roi.rect.w(), oh, ow);
    if (int rc = launch_dec_out_frame(staged_frame(f, oh, ow), synout, h, w, false, true, s)) return rc;
    if (f.tone)
        if (int rc = launch_dec_tone_frame(*f.tone, oh, ow, s)) return rc;
    if (dec_flt_class(f) == 2) return CCMI_OK; // mix-staged, nothing to filter: dec_mix_batch reads the staged frame
    const DecFltEntry F = filter_entry(f);
    const int tiles_x = filter_tiles_x(ow);
    const dim3 grid((unsigned)(tiles_x * filter_tiles_y(oh)));
    if (f.mix) { // mix-staged: filtered in float32 into its second frame
        hipLaunchKernelGGL(dec_filter<float>, grid, dim3(kThreads), 0, s, F, oh, ow, identity_call(oh, ow), tiles_x);
        CCMI_HIP_CHECK(hipGetLastError());
        return CCMI_OK;
    }
    const DecFmtCall C = fmt_call(f.fmt);
    return with_elem_type(f.fmt.elem, [&](auto t) {
        hipLaunchKernelGGL(dec_filter<decltype(t)>, grid, dim3(kThreads), 0, s, F, oh, ow, C, tiles_x);
    });
}

} // namespace ccmi
