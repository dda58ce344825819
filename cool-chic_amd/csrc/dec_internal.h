// dec_internal.h -- path B (fixed-point .cool decoder) shared definitions.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "ccmi_internal.h"

namespace ccmi {

constexpr int kArmPrec = 8;  // ARM_PRECISION   (coolchic/cpp/common.h:26)
constexpr int kUpsPrec = 12; // UPS_PRECISION   (common.h:29)
constexpr int kSynPrec = 12; // SYN_*_PRECISION (common.h:31-34)

struct SynLayerDesc {
    int n_out, ks, residual, relu;
};

// One intra frame of a .cool stream, parsed and with its networks decoded to the
// fixed-point integers the kernels use (host side).
struct FrameHost {
    // GOP header (cc-bitstream.cpp:58-84)
    int h = 0, w = 0, bitdepth = 8, frame_data_type = 0, intra_period = 0;
    // frame header (cc-bitstream.cpp:140-234)
    int dim_arm = 0, n_hidden = 0;
    int n_ups = 0, ups_ks = 0, n_pre = 0, pre_ks = 0;
    int n_branches = 1;
    std::vector<SynLayerDesc> layers;
    int sig_blk = 0;
    int n_layers = 0;
    int lh[CCMI_MAX_GRIDS] = {}, lw[CCMI_MAX_GRIDS] = {};
    const uint8_t *lat_bytes[CCMI_MAX_GRIDS] = {};
    uint32_t lat_n[CCMI_MAX_GRIDS] = {};
    // network substreams (arm w / b, ups w, syn w / b) and their q-step records (qw, qb, sw,
    // sb, nw, nb for arm / ups / syn), kept by the header parse for decode_frame_weights
    const uint8_t *wbytes[5] = {};
    int lqi[3][6] = {};
    // decoded networks
    std::vector<int32_t> arm;   // per hidden layer: W[d][d] (out, in) then b[d]; then Wout[2][d], bout[2]
    std::vector<int32_t> ups;   // n_ups kernels of ups_ks taps, then n_pre kernels of pre_ks taps (mirrored)
    std::vector<int32_t> syn;   // per branch, per layer: W[n_out][n_in][ks][ks] then b[n_out]
    std::vector<int32_t> blend; // n_branches values when n_branches > 1
    bool fusable_head() const { return layers.size() >= 2 && layers[0].ks == 1 && layers[1].ks == 1; }
};

// Parses the GOP + first frame of `bs` and decodes its weights.  Returns CCMI_OK or an
// error code (message set).  Pointers in `f` alias `bs`.
int parse_and_decode_frame(const uint8_t *bs, size_t n, FrameHost &f);
// The two halves: headers only (geometry, architecture, substream sizes; the weight arrays
// sized, not filled) -- enough to plan memory and output sizes -- then the CABAC decode of
// the network weights.
int parse_frame_header(const uint8_t *bs, size_t n, FrameHost &f);
int decode_frame_weights(FrameHost &f);

// Descriptor of one latent-layer CABAC stream for the ARM decode kernel.
struct ArmStreamDesc {
    const uint32_t *bytes; // device, zero-padded to a multiple of 16 bytes
    uint32_t nbytes;
    int h, w, sig_blk;
    int d, nh;
    int flags;              // bit 0: every ARM weight fits in 24 signed bits
    const int32_t *weights; // device copy of FrameHost::arm
    int32_t *out;           // device h*w plane, value << kArmPrec
    uint64_t *dbg;          // diagnostic builds only (CCMI_ARM_STAMPS): 8 counters per stream
    uint32_t *status;       // device word, zeroed by the host: CCMI_ARM_FLAG_* bits OR-ed in by the kernel
    int spin_cap;           // chain kernel: polls per wait before it gives up and flags CCMI_ARM_FLAG_TIMEOUT
    // rows [0, rows) are decoded and written (a region decode stops below the last row its
    // window reads); rows == h for a whole frame.  The block maps are decoded up front and
    // use the true h.
    int rows;
};

// One launch for n_streams streams sharing (d, nh); max_w / max_blocks size the LDS
// ring and the block map.
int launch_dec_arm(const ArmStreamDesc *d_streams, int n_streams, int max_w, int max_blocks, int d, int nh,
                   hipStream_t s);

// Upsampling of one frame: latent planes (int32, flat) -> [L][H][W] at UPS precision.
struct DecUpsArgs {
    const int32_t *lat; // flat: grid l at off[l]
    int n_layers;
    int lh[CCMI_MAX_GRIDS], lw[CCMI_MAX_GRIDS], off[CCMI_MAX_GRIDS];
    const int32_t *kernels; // device copy of FrameHost::ups
    int ups_ks, n_ups, pre_ks, n_pre;
    int32_t *workspace;     // stacks of levels 1..L-2
    int32_t *out;           // [L][H][W]
};
size_t dec_ups_workspace_elems(const int *lh, const int *lw, int L);
int launch_dec_ups(const DecUpsArgs &a, hipStream_t s);

// Synthesis of one frame (single branch): [C][H][W] at 12-bit -> [C_out][H][W].
struct DecSynArgs {
    const int32_t *in;
    int c_in, h, w;
    int n_layers;
    SynLayerDesc layers[CCMI_MAX_SYN_LAYERS];
    const int32_t *params; // per layer W then b (one branch)
    int32_t *out;
    int32_t *workspace;    // generic path ping-pong, 2 * maxc * h * w
    // every weight fits 24 signed bits (host-checked): the fused kernel multiplies with
    // v_mul_i32_i24 (full rate) instead of v_mul_lo_u32 (quarter rate).  The activations
    // always fit: each is an int32 shifted right by UPS_/SYN_ precision 12 (|v| <= 2^19), and
    // a 24x24-bit product's low 32 bits equal the int32 product's.
    int f24 = 0;
};
size_t dec_syn_workspace_elems(const DecSynArgs &a);
int launch_dec_syn(const DecSynArgs &a, hipStream_t s);

// Multi-branch blend (synblend_cpu.hpp): first: acc = (clamp(acc)*b0 + clamp(x)*b1) >> 12,
// later: acc += (clamp(x) * bk) >> 12; 3 planes.
int launch_dec_blend(int32_t *acc, const int32_t *x, int64_t n, int32_t b_acc, int32_t b_x, int first,
                     hipStream_t s);

// A rectangle of one pyramid level, [y0, y1) x [x0, x1) in that level's coordinates.
struct DecWindow {
    int y0, y1, x0, x1;
    int h() const { return y1 - y0; }
    int w() const { return x1 - x0; }
};
// What a region decode of one frame computes: rect = the region (level-0 coordinates);
// lev[k] = the window of pyramid level k the region needs (lev[0]: the synthesis input,
// the region grown by the 3x3 layers' reach and clipped to the frame); arm_rows[l] = the
// rows of latent grid l those windows read; lat[l] = the rectangle of grid l they read (grid
// l < L-1: lev[l] grown by the refine's pre_ks / 2 on every side, clipped to the plane; the
// coarsest grid: lev[L-1]), which is what a render from a latent store unpacks.  Planned on
// the host (dec_roi_plan).
struct DecRoi {
    DecWindow rect;
    DecWindow lev[CCMI_MAX_GRIDS];
    int arm_rows[CCMI_MAX_GRIDS];
    DecWindow lat[CCMI_MAX_GRIDS];
};
// syn_halo: the sum of (ks - 1) / 2 over the synthesis layers
void dec_roi_plan(const int *lh, const int *lw, int L, int ups_ks, int pre_ks, int syn_halo, const DecWindow &rect,
                  DecRoi &r);
size_t dec_ups_workspace_elems_win(const DecRoi &r, int L); // the stacks of levels 1..L-2, windows only

// Formatted tensor output (ccmi_tensor_fmt, validated and resolved by the plan): three full-size
// channels per pixel, colour, affine, element type, strides and mirror applied by the output
// kernel (dec_fmt<Plain, T, TABLE>, dec_out.hip).  Everything but `matrix` and `mirror` is one value per call.
struct DecFmt {
    int on = 0;     // 0: the planar u8 / u16 / f32 tensor output
    int elem = 0;   // CCMI_ELEM_*
    int matrix = 0; // this frame takes the YUV -> RGB matrix (CCMI_COLOUR_RGB on a YUV stream)
    int mirror = 0; // this frame's destination x is reversed
    float scale[3] = {1.f, 1.f, 1.f}, bias[3] = {0.f, 0.f, 0.f};
    int64_t stride_c = 0, stride_y = 0, stride_x = 0; // elements, resolved (never all 0)
    // ccmi_resample (one per call): the region, of any size, is resampled to out_h x out_w between
    // the colour step and scale / bias (dec_resize_h<CUBIC>, dec_fmt<Resize<CUBIC>, T, TABLE>); strides and mirror
    // then refer to the output size
    int rs = 0;
    int out_h = 0, out_w = 0;
    // ccmi_warp: every out_h x out_w output pixel is a bilinear sample of the whole frame at the
    // position this frame's matrix m gives (dec_fmt<Warp<CUBIC, PERSP>, T, TABLE>), between the same two steps; pad and
    // fill are one per call.  Never together with rs
    int warp = 0;
    int pad = 0;
    float fill[3] = {0.f, 0.f, 0.f};
    float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    // CCMI_WARP_PROJECTIVE (one per call): m is the frame's 3 x 3 homography and the position the
    // quotient by its third row (Warp<CUBIC, true>); without it m[6 .. 8] are unused
    int persp = 0;
    // CCMI_FILTER_CUBIC / CCMI_WARP_CUBIC (one per call): the cubic forms of the rs / warp kernels
    // (Resize<true>, Warp<true, PERSP>); clamp: their r' is clamped to [0, 1].  pad is
    // CCMI_PAD_FILL or CCMI_PAD_EDGE, without the flags
    int cubic = 0, clamp = 0;
    // ccmi_colour with at least one op in the call (one value per call): the colour forms of the
    // output kernels run, each frame with its own DecCol (DecTailFrame::col), after any of the above
    int col = 0;
};
// ccmi_colour of one frame (step 3z of the contract in ccmi.h), validated and resolved by the plan:
// the op table the colour forms of the output kernels read from the tail's argument tables.
struct DecColOp {
    int op;      // CCMI_COL_*
    float v[12]; // v[0] = f and, SATURATION / CONTRAST, v[1] = 1 - f (float32, computed once here); MATRIX: M
};
struct DecCol {
    int n = 0;         // ops
    int contrast = -1; // the index of the frame's contrast op, or -1
    // device: the frame's S_j in the workspace (decode_run), cleared in stream and summed by the
    // statistics pass before the output kernel reads it; unused without a contrast op
    unsigned long long *acc = nullptr;
    DecColOp ops[CCMI_COL_MAX_OPS] = {};
};

// ccmi_filter of one frame that takes the stage (steps 3y-0 .. 3y-2 of the contract in ccmi.h),
// validated and resolved by the plan.  The frame's geometry and colour kernels write it in the identity
// format into `tmp`; the filter kernel (dec_filter.hip) reads it there and writes the caller's tensor.
struct DecFlt {
    int r = 0;       // radius; 0: solarize only
    int sol = 0;     // the threshold acts (th <= 1)
    float th = 0.f;
    float taps[CCMI_FLT_MAX_RADIUS + 1] = {}; // w_0 .. w_r
};
// what the stage adds to the call's tables per staged frame: the frame's entry of the staging launch,
// its filter entry and the taps in it (the workspace formula of ccmi.h)
constexpr size_t kFltTableBytes = 256;

// ccmi_tone of one staged frame (step 3x of the contract in ccmi.h), validated and resolved by the
// plan; with device pointers filled by decode_run it is also the frame's entry of the tone tables the
// kernels of dec_tone.hip read.  A call with a tone op has one for EVERY staged frame (n == 0: the
// frame leaves every pass at once).  The list is cut into segments: a run of pointwise ops ended by
// a whole-frame op (its terminator) or by the end of the list.
struct DecToneOp {
    int op;      // CCMI_TONE_*
    float v[12]; // v[0] = f / th and, factors, v[1] = 1 - f; POSTERIZE: L, 1 / L, L - 1; MATRIX: M
};
struct DecToneSeg {
    uint8_t first, end; // the segment's pointwise ops [first, end)
    uint8_t term;       // its terminator's op code (ops[end]), or kToneNoTerm
    uint8_t src;        // which of buf[] holds the frame when the segment starts
    uint8_t acc;        // the terminator's accumulator block, counted from the frame's first
    uint8_t pad_[3];
};
constexpr int kToneNoTerm = 255;
struct DecTone {
    float *buf[2] = {nullptr, nullptr}; // device: the staging frame and, with a sharpness op, the second frame
    uint8_t *acc = nullptr;             // device: the frame's accumulator blocks, kToneAccBytes each
    int n = 0, nseg = 0;
    DecToneSeg seg[CCMI_TONE_MAX_OPS] = {};
    DecToneOp ops[CCMI_TONE_MAX_OPS] = {};
};
static_assert(sizeof(DecTone) == 512, "kToneTableBytes per staged frame");
// per staged frame of a call with a tone op, after the group's kFltTableBytes each
constexpr size_t kToneTableBytes = 512;
// one accumulator block: 3 x 256 bins, 3 complemented minima, 3 maxima (float bits), one 64-bit sum
constexpr size_t kToneAccHist = 0, kToneAccMin = 3072, kToneAccMax = 3084, kToneAccSum = 3096, kToneAccBytes = 3328;
inline int dec_tone_sharps(const DecTone &t)
{
    int k = 0;
    for (int i = 0; i < t.n; ++i) k += t.ops[i].op == CCMI_TONE_SHARPNESS;
    return k;
}
inline int dec_tone_stats(const DecTone &t)
{
    int k = 0;
    for (int i = 0; i < t.n; ++i)
        k += t.ops[i].op == CCMI_TONE_CONTRAST || t.ops[i].op == CCMI_TONE_AUTOCONTRAST || t.ops[i].op == CCMI_TONE_EQUALIZE;
    return k;
}
// the table bytes of a staged frame: with a tone op in the call, its DecTone follows
inline size_t dec_flt_table_bytes(bool tone) { return kFltTableBytes + (tone ? kToneTableBytes : 0); }

// ccmi_mix of one frame (steps 4e and 4m of the contract in ccmi.h), validated and resolved by the plan.
// A mix-staged frame takes the filter stage, which leaves it in float32 in the workspace (the staging
// frame, or DecTailFrame::mix_buf where the filter kernel has something to compute); dec_mix_batch
// (dec_mix.hip) then formats all of them in one launch from the call's mix table.
struct DecMixRect {
    int x, y, w, h;
    float v[3], sigma;
};
struct DecMix {
    int staged = 0;    // the frame is mix-staged: it takes the stage or is the partner of a frame that does
    int entry = -1;    // staged: its entry of the mix table
    int count = 0;     // rectangles
    int partner = -1;  // a frame of the call, or -1
    float lam = 1.f, oml = 0.f; // lam and 1.0f - lam (float32, computed once here)
    int box[4] = {0, 0, 0, 0};  // x, y, w, h; w == 0: no box (a blend)
    uint64_t seed = 0;
    DecMixRect r[CCMI_MIX_MAX_RECTS] = {};
};
// what the stage adds to the call's tables per mix-staged frame (the workspace formula of ccmi.h)
constexpr size_t kMixTableBytes = 256;

// ccmi_blend of one frame (step 3b of the contract in ccmi.h), validated by the plan.  A blend-staged frame
// (terms, silent, or a source) is mix-staged: its DecMix is staged and has an entry.  The terms travel in
// the blend table, the sibling of the mix table that follows it: kBlendTableBytes per mix-staged frame, the
// whole rounded up to 256; dec_blend_batch (dec_blend.hip) is then the call's one launch.
struct DecBlend {
    int count = 0;  // terms
    int silent = 0; // rendered and staged, no output
    int src[CCMI_BLEND_MAX_TERMS] = {}; // frames of the call
    float w[CCMI_BLEND_MAX_TERMS] = {};
};
constexpr size_t kBlendTableBytes = 64;
inline size_t dec_blend_table_bytes(int n_mix) { return (kBlendTableBytes * (size_t)n_mix + 255) / 256 * 256; }

// the form of a tail group's output section: the plain entry, or its resample / warp / projective warp extension
enum { kOutPlain = 0, kOutRs = 1, kOutWarp = 2, kOutPersp = 3 };
inline int dec_out_form(const DecFmt &f) { return f.rs ? kOutRs : f.warp ? (f.persp ? kOutPersp : kOutWarp) : kOutPlain; }
// a resample's horizontal pass (DecTailFrame::rs_tmp), in floats
size_t dec_resample_tmp_elems(int region_h, int out_w);

// Batched decoder tail: frames with the same geometry and a fused-synthesis architecture
// (single branch) share one launch per pyramid step, one synthesis and one output launch
// (grid.y = frame) instead of ~8 launches per frame.  The per-frame argument tables live
// in device memory: dec_tail_table_bytes() sizes them, dec_tail_fill() writes them on the
// host (device pointers inside), the caller uploads them, launch_dec_tail_batch() runs.
struct DecTailFrame {
    DecUpsArgs ups;
    DecSynArgs syn;
    int bitdepth, kind;
    uint8_t *dst;
    int sample = -1; // -1: file bytes at dst (workspace staging); CCMI_SAMPLE_*: planar tensor at dst (caller's)
    DecFmt fmt;      // fmt.on: the formatted tensor at dst instead (sample is then CCMI_SAMPLE_F32, unused)
    float *rs_tmp = nullptr; // fmt.rs: the frame's horizontal-pass intermediate, [3][region h][out_w]
    const DecCol *col = nullptr; // fmt.col: the frame's colour ops (n == 0: none), in DecodePlan::cols
    // the frame takes the filter stage: its DecFlt (in DecodePlan::flts) and its float32 staging
    // frame, [3][oh][ow] of the stored frame
    const DecFlt *flt = nullptr;
    float *flt_tmp = nullptr;
    // ccmi_tone with an op in the call: every staged frame's DecTone (in DecodePlan::tones; device
    // pointers set by decode_run), NULL otherwise
    const DecTone *tone = nullptr;
    // ccmi_mix: the frame is mix-staged (its DecMix, in DecodePlan::mixes; NULL otherwise): the filter
    // kernel does not write `dst` -- with a radius or a solarize it writes mix_buf, [3][oh][ow] float32 in
    // the identity format, and otherwise it is not launched for the frame -- and dec_mix_batch does
    const DecMix *mix = nullptr;
    float *mix_buf = nullptr;
    // region decode on windows: the latent planes keep their frame pitch and hold roi.arm_rows[l]
    // rows, ups.workspace / ups.out / syn.out hold the windows roi.lev[k] / the region, compact
    // (pitch = the window's width); ups.lh / lw and syn.h / w stay the frame's true sizes
    bool windowed = false;
    DecRoi roi{};
};
bool dec_tail_batchable(const DecTailFrame &f);
bool dec_tail_same_group(const DecTailFrame &a, const DecTailFrame &b);
// col: the group's frames carry a DecCol each, a fourth section of the table
size_t dec_tail_table_bytes(int n_layers, int n, bool windowed = false, int out_form = kOutPlain, bool col = false);
// n_flt: the LAST n_flt frames of the group take the filter stage (DecTailFrame::flt); flt_tab is
// their part of the call's filter tables, kFltTableBytes per frame (dec_flt_fill)
void dec_tail_fill(const DecTailFrame *const *fr, int n, void *host_tab, int n_flt = 0, void *host_flt_tab = nullptr);
// fr: the group's frames, in table order (a window-form group sizes its grids by their windows)
int launch_dec_tail_batch(const DecTailFrame *const *fr, int n, const void *dev_tab, hipStream_t s, int n_flt = 0,
                          const void *dev_flt_tab = nullptr);

// The output stage (dec_out.hip), all the tail knows of it: synthesis output (12-bit, [3][h][w])
// to file bytes (sample < 0; ccdecapi.cpp:59-240; kind 0 yuv420, 1 yuv444, 2 ppm payload), to the
// planar tensor (kind 0 Y[H][W] U V [H/2][W/2], kind 1 [3][H][W]; dst needs one sample's
// alignment only) or, with fmt.on, to the formatted tensor -- resampled (fmt.rs), warped
// (fmt.warp) and through the frame's colour ops (fmt.col, after the statistics pass where a
// frame has a contrast op; DecCol::acc is cleared by the caller, in stream) on the way.
// A tail group's output section holds one entry per frame, of its out_form's size ...
size_t dec_out_entry_bytes(int out_form);
// ... and dec_out_fill writes entry i of it (host side), and of the colour section with fmt.col,
// for the frame's h x w synthesis output that sits at (oy, ox) of its frame.
void dec_out_fill(void *out_sec, void *col_sec, int i, const DecTailFrame &f, int h, int w, int oy, int ox);
// The output stage of a group of n frames like f0, from the uploaded sections: h x w is the
// synthesis output (a window-form group's: the largest region); stat: a frame has a contrast op.
int launch_dec_out_group(const DecTailFrame &f0, int h, int w, int n, const void *out_sec, const DecCol *col_sec,
                         bool stat, hipStream_t s);
// The output stage of one frame (the per-frame tail) from its whole-frame h x w synthesis output.
// Formatted: the region f.roi.rect (kind 0: an even origin), a warp the whole frame (kind 0: h and
// w even).  Planar: crop takes f.roi.rect, else device the whole frame; neither: file bytes.
int launch_dec_out_frame(const DecTailFrame &f, const int32_t *synout, int h, int w, bool crop, bool device,
                         hipStream_t s);

// The filter stage (dec_filter.hip).  The staged frames of a group, m of them, have their own tables,
// kFltTableBytes per frame: [m] entries of the group's out_form for the staging launch (the frames'
// entries with dst = the staging frame), then [m] filter entries.  dec_flt_fill writes frame i's of
// both (host side; h, w, oy, ox as for dec_out_fill).  With a tone op in the call (f.tone) the group's
// table is dec_flt_table_bytes(true) per frame and [m] DecTone follow at kFltTableBytes * m.
void dec_flt_fill(void *flt_tab, int m, int i, const DecTailFrame &f, int h, int w, int oy, int ox);
// The output stage of the m staged frames fr[0 .. m) of a group: the group's output kernels in the
// identity format into the staging frames (h x w and col_sec as for launch_dec_out_group, col_sec
// being the first staged frame's entry), then dec_filter_batch into the caller's tensors.
int launch_dec_out_group_flt(const DecTailFrame *const *fr, int m, int h, int w, const void *dev_flt_tab,
                             const DecCol *col_sec, hipStream_t s);
// launch_dec_out_frame for a frame that takes the stage (f.flt): staged, then dec_filter.
int launch_dec_out_frame_flt(const DecTailFrame &f, const int32_t *synout, int h, int w, hipStream_t s);

// The frames of a group that take the filter stage run in this order (build_tail_groups sorts them so):
// 0, formatted to the caller's tensor by the filter kernel; 1, mix-staged with a radius or a solarize
// (the filter kernel writes mix_buf); 2, mix-staged without (no filter launch).
inline int dec_flt_class(const DecTailFrame &f) { return !f.mix ? 0 : (f.flt && (f.flt->r > 0 || f.flt->sol)) ? 1 : 2; }
// where a mix-staged frame stands in float32 once its tail has run: what dec_mix_batch reads
const float *dec_mix_source(const DecTailFrame &f);

// The mix stage (dec_mix.hip): the call's mix table, kMixTableBytes per mix-staged frame.  dec_mix_fill
// writes entry f.mix->entry (host side; the device pointers are the frame's and its partner's,
// partner_entry the partner's entry or -1), launch_dec_mix formats the n_entries frames in one launch
// per 65535 of them; fmt: any of the frames' (element type, scale and bias are one per call; the resolved
// strides are each frame's own and travel in its entry), max_oh x max_ow: the largest stored frame among them.
void dec_mix_fill(void *host_tab, const DecTailFrame &f, int oh, int ow, int partner_entry);
int launch_dec_mix(const void *dev_tab, int n_entries, int max_oh, int max_ow, const DecFmt &fmt, hipStream_t s);
// ccmi_blend: after dec_mix_fill, the terms of entry `entry` (src_entries: the sources' entries of the mix
// table) into both host tables, and no destination for a silent frame; launch_dec_blend is launch_dec_mix
// for a call with a blend table (dec_blend_batch: K sources per frame, silent entries leave at once)
void dec_blend_fill(void *host_mix_tab, void *host_blend_tab, int entry, const DecBlend &b, const int *src_entries);
int launch_dec_blend(const void *dev_mix_tab, const void *dev_blend_tab, int n_entries, int max_oh, int max_ow,
                     const DecFmt &fmt, hipStream_t s);

// The tone stage (dec_tone.hip), between the staging launches and the filter launch: segment after
// segment, a statistics pass where a frame's terminator needs one, then the apply pass (in place) or
// the sharpness pass (into the frame's other buffer).  es: the m entries in device memory, host: the
// same on the host (the passes to launch are read off them).  The accumulators are cleared by the caller.
int launch_dec_tone_group(const DecTone *dev_es, const DecTone *const *host, int m, int oh, int ow, hipStream_t s);
// one frame, its entry as the kernels' own argument (the per-frame tail)
int launch_dec_tone_frame(const DecTone &e, int oh, int ow, hipStream_t s);

// Latent store (dec_latents.hip): the ARM output planes (int32, value << kArmPrec) packed to
// values of the store's element type (CCMI_LATENT_*), and back.  Both kernels are table-driven:
// a job owns the blocks [first_block, the next job's first_block) of the launch; the tables
// live in device memory and are filled on the host.
struct DecLatPackJob {
    const int32_t *src;   // 16-byte aligned
    void *dst;            // 16-byte aligned, n values
    uint32_t *status;     // the grid's status word: CCMI_ARM_FLAG_NARROW is OR-ed in on a misfit
    uint32_t n;
    uint32_t first_block;
    int shift;            // kArmPrec for latent planes; 0: a plain int32 copy (the networks' integers)
    int pad_;
};
struct DecLatUnpackJob {
    const void *src;      // the grid's packed values, whole plane, pitch w; NULL: an all-zero grid
    int32_t *dst;         // plane at pitch w
    int w;
    int y0, y1, x0, x1;   // the rectangle to write
    uint32_t first_block;
    int shift;            // kArmPrec for the tail's planes; 0: the values themselves
    int h;                // the plane's rows (CCMI_LATENT_SEG: the payload follows the h * nseg descriptors)
};
size_t dec_lat_elem_bytes(int type); // 0: not one of CCMI_LATENT_I8 / I16 / I32
uint32_t dec_lat_pack_blocks(uint32_t n, int type);
uint32_t dec_lat_unpack_blocks(const DecWindow &r);
// jobs: device table of n_jobs entries whose first_block counts from 0; n_blocks = their total
int launch_dec_lat_pack(const DecLatPackJob *jobs, int n_jobs, uint32_t n_blocks, int type, hipStream_t s);
// type CCMI_LATENT_SEG: dec_lat_unpack_seg, src = the grid's descriptor table
int launch_dec_lat_unpack(const DecLatUnpackJob *jobs, int n_jobs, uint32_t n_blocks, int type, hipStream_t s);

// Segmented form (CCMI_LATENT_SEG, the contract in ccmi.h): a grid is rows of segments of
// kSegLen values, each at the narrowest of six widths; a descriptor table, then the payload.
// Compaction of a built store runs three table-driven kernels, one job per non-empty grid, one
// wave per segment: the width pass writes the segment's code to the job's words of the
// workspace, the scan (one block per grid) turns them into descriptors in place and writes the
// grid's payload words to totals[job], the pack writes descriptors and payload to the new store.
constexpr int kSegLen = 64;
constexpr uint32_t kSegOffMax = (1u << 29) - 1;   // a descriptor's word offset has 29 bits
constexpr uint32_t kSegTotalBad = 0xFFFFFFFFu;    // totals[job]: a segment's offset does not fit
struct DecLatSegJob {
    const void *src;      // the source grid's values (elem bytes each), whole plane, pitch w
    uint32_t *desc;       // workspace, h * nseg words: width codes, then descriptors
    uint32_t *desc_out;   // pack: the new store's descriptor table
    uint32_t *payload;    // pack: the new store's payload words
    int w, h, nseg;
    int elem;             // 1, 2 or 4 bytes per source value
    uint32_t first_seg;   // of the launch's segments, this grid's first
    uint32_t pad_;
};
inline uint32_t dec_lat_seg_per_row(int w) { return (uint32_t)((w + kSegLen - 1) / kSegLen); }
inline size_t dec_lat_seg_table_bytes(int h, int w) // the descriptor table, 16-byte aligned
{
    return ((size_t)h * dec_lat_seg_per_row(w) * 4 + 15) & ~(size_t)15;
}
// jobs: device table ordered by first_seg, n_segs = their total
int launch_dec_lat_seg_width(const DecLatSegJob *jobs, int n_jobs, uint32_t n_segs, hipStream_t s);
int launch_dec_lat_seg_scan(const DecLatSegJob *jobs, int n_jobs, uint32_t *totals, hipStream_t s);
int launch_dec_lat_seg_pack(const DecLatSegJob *jobs, int n_jobs, uint32_t n_segs, hipStream_t s);

// Latent-store files (dec_store_file.cpp, the contract in ccmi.h).  Three more table-driven
// kernels: the gather copies a defined byte range of a store to its place in the DATA image
// (src and dst 16-byte aligned, n of any size), the checksum adds a range's two sums to
// sum[0..1] (zeroed by the host; integer sums, so the order of the blocks does not matter), the
// verify (one block per non-empty SEG grid) checks an untrusted descriptor table against the
// payload size its record states and writes the grid's status word (0, or kSegBad* bits).
struct DecLatGatherJob {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t n;           // bytes
    uint32_t first_block;
    uint32_t pad_;
};
struct DecLatSumJob {
    const uint32_t *src;  // 16-byte aligned
    unsigned long long *sum;
    uint64_t n_words;
    uint32_t first_block;
    uint32_t pad_;
};
struct DecLatVerifyJob {
    const uint32_t *desc; // the grid's h * nseg descriptors
    uint32_t *status;
    int w, h, nseg;
    uint32_t seg_words;   // the payload words the record states
};
enum { kSegBadCode = 1, kSegBadOffset = 2, kSegBadTotal = 4 };
uint32_t dec_lat_gather_blocks(uint64_t n_bytes);
uint32_t dec_lat_sum_blocks(uint64_t n_words);
int launch_dec_lat_file_gather(const DecLatGatherJob *jobs, int n_jobs, uint32_t n_blocks, hipStream_t s);
int launch_dec_lat_file_sum(const DecLatSumJob *jobs, int n_jobs, uint32_t n_blocks, hipStream_t s);
int launch_dec_lat_seg_verify(const DecLatVerifyJob *jobs, int n_jobs, hipStream_t s);

} // namespace ccmi
