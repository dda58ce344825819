// dec_plan.h -- path B: what one decode call asks for (DecodeRequest) and what the header
// pass makes of it (DecodePlan).  decode_plan() is host arithmetic on header fields of
// untrusted streams and makes no HIP call; decode_run() (dec_host.cpp) executes a plan.
#pragma once

#include "dec_internal.h"

namespace ccmi {

// One stream of a latent store (ccmi_latents): what a render needs of it on the host, the form
// of its latents, and where its parts sit in its device store (bytes from `base`: a handle made
// by ccmi_latents_concat spans several stores).
struct LatentStream {
    FrameHost f;  // header facts and decoded networks; refers to no coded bytes (pointers cleared, ARM dropped)
    int f24 = 0;  // DecSynArgs::f24, computed once at the build
    int type = 0; // CCMI_LATENT_*
    const uint8_t *base = nullptr; // device: the store this stream sits in; NULL: plan-only
    size_t off = 0, bytes = 0; // the stream's part of the store, 256-byte aligned and rounded
    size_t ups_off = 0, syn_off = 0;
    // an empty grid (lat_n == 0) takes no bytes; CCMI_LATENT_SEG: the descriptor table, the payload
    // dec_lat_seg_table_bytes() behind it
    size_t grid_off[CCMI_MAX_GRIDS] = {};
    // CCMI_LATENT_SEG: the payload words of each non-empty grid (the compaction's scan, or a
    // file's record); grid_off differences do not give the last grid's, the part being rounded
    uint32_t seg_words[CCMI_MAX_GRIDS] = {};
};

} // namespace ccmi

// The opaque handle of ccmi.h: immutable once built.  Type and store are per stream; every
// stream of a handle is resident, or none is (plan-only).
struct ccmi_latents {
    bool resident = false;
    size_t store_bytes = 0; // the sum of the streams' bytes
    std::vector<ccmi::LatentStream> s;
};

namespace ccmi {

enum OutKind { kYuv420 = 0, kYuv444 = 1, kPpm = 2 };

struct OutFmt {
    int kind, bitdepth;
    size_t payload, header;
    char hdr[48];
};

// file layout of a host-byte sink (PPM, or planar YUV when as_yuv)
int out_format(const FrameHost &f, int out_bitdepth, int out_chroma, int as_yuv, OutFmt &o);

// how a stream's decoder tail runs
enum TailMode {
    kTailFrame = 0,  // the whole frame (no region, or one that covers the frame)
    kTailWindow = 1, // region decode on windows (batched tail, fused synthesis)
    kTailCrop = 2,   // whole-frame per-frame tail, the region cropped by the output kernel
};

// One call of the decode driver.  The sink is host bytes (the default): file layout, staged
// in the workspace and copied to outs[i]; or device tensors (sample >= 0): the output kernel
// writes planar samples of type `sample` straight to dev[i], nothing is staged and nothing
// is downloaded (with fmt: the formatted tensor instead); or a latent store (lat_store): no
// decoder tail at all, the ARM output planes are packed into the store.  outs / dev NULL:
// planning only.
// The source is coded streams, or (src) streams of a latent store: frame i is stream index[i]
// of the handle, the ARM stage is replaced by an unpack of the store, and n counts frames.
struct DecodeRequest {
    const uint8_t *const *streams = nullptr;
    const size_t *lens = nullptr;
    int n = 0;
    int out_bitdepth = 0, out_chroma = 0; // 0: the stream's own
    // host-byte sink
    int as_yuv = 0;
    uint8_t *const *outs = nullptr; // [n] host buffers
    // device-tensor sink
    int sample = -1;               // -1 host bytes, else CCMI_SAMPLE_*
    void *const *dev = nullptr;    // [n] device pointers
    const ccmi_rect *roi = nullptr; // [n], optional: the region of each frame to decode
    // formatted device-tensor sink (ccmi_tensor_fmt): three full-size channels, colour, affine,
    // element type, strides and mirror; sample is CCMI_SAMPLE_F32 (the workspace is that call's)
    const ccmi_tensor_fmt *fmt = nullptr;
    // with fmt, optional: every frame's region is resampled to one output size (ccmi_resample)
    const ccmi_resample *rs = nullptr;
    // with fmt, instead of roi and rs: every output pixel samples the whole frame through the
    // frame's matrix (ccmi_warp); the plan derives each frame's region, its window, from the matrix
    const ccmi_warp *warp = nullptr;
    ccmi_rect *window = nullptr; // [n], optional: the windows, filled by the plan
    // with fmt, optional: every frame's own list of colour ops between the geometry and scale / bias
    // (ccmi_colour); with an op in any frame the call runs the colour forms of the output kernels
    const ccmi_colour *colour = nullptr;
    // with fmt, optional: per-frame blur taps and solarize thresholds after the colour ops (ccmi_filter);
    // the frames that take the stage are staged in float32 and go through the filter kernel
    const ccmi_filter *filter = nullptr;
    // with fmt, optional: per-frame lists of tone ops on the staged frame, after the colour ops and before
    // the filter (ccmi_tone); a frame with a list takes the filter's stage
    const ccmi_tone *tone = nullptr;
    // with fmt, optional: per-frame erase rectangles, partners, blend weights and boxes (ccmi_mix); the
    // mix-staged frames take the filter's stage and are formatted by the call's one mix launch
    const ccmi_mix *mix = nullptr;
    // with fmt, optional: per-frame weighted sums of staged frames and silent frames (ccmi_blend); the
    // blend-staged frames are mix-staged and the call's one launch is dec_blend_batch
    const ccmi_blend *blend = nullptr;
    // either sink
    const size_t *caps = nullptr;    // [n], optional: capacity in bytes of outs[i] / dev[i]
    size_t *sizes = nullptr;         // [n], optional: bytes written per stream (filled by the plan)
    ccmi_frame_geom *geom = nullptr; // [n], optional (device sinks): filled by the plan
    ccmi_roi_info *info = nullptr;   // [n], optional (device sinks): what the region decode does
    int32_t *const *lat_out = nullptr; // [n], optional: the decoded latents, to the host
    // latent-store sink: the layout is filled by the plan; !lat_store->resident: planning only
    ccmi_latents *lat_store = nullptr;
    // latent-store source
    const ccmi_latents *src = nullptr;
    const int *index = nullptr; // [n], optional: NULL = frame i is stream i (n == the handle's count)
    // caller-owned device workspace (NULL: one hipMalloc per call)
    void *ws = nullptr;
    size_t ws_bytes = 0;
    bool device() const { return sample >= 0; }
};

// One stream of a call.  Offsets are bytes from the workspace base.
struct FramePlan {
    FrameHost f;
    OutFmt of;
    int mode = kTailFrame;
    bool batchable = false; // single branch and an architecture the batched tail takes
    bool arm24 = false;     // every ARM weight fits 24 signed bits (decode_run, once they are decoded)
    int src = -1;           // latent-store source: the handle's stream this frame renders
    bool silent = false;    // ccmi_blend: rendered and staged, no output (set before the frame is planned)
    // tail arguments: architecture, output format and region (tail.roi) from the plan, device
    // pointers and syn.f24 from decode_run
    DecTailFrame tail;
    // constant part (uploaded): coded bytes per latent grid, then the three networks
    size_t bytes_off[CCMI_MAX_GRIDS];
    size_t arm_off, ups_off, syn_off;
    // scratch
    size_t lat_off, ws_off, dense_off, synout_off, synws_off, out_off;
    size_t lat_elems, ws_elems, dense_elems, synout_elems, synws_elems;
    size_t rs_off = 0, rs_elems = 0; // a resample's horizontal-pass intermediate (float32); none without one
    size_t flt_off = 0, flt_elems = 0; // the filter stage's staging frame (float32); none unless the frame takes it
    size_t tone2_off = 0;              // ccmi_tone: a second frame of flt_elems for a list with a sharpness op
    size_t tone_acc_off = 0;           // ccmi_tone: the frame's accumulator blocks, one per statistic op
    size_t mix2_off = 0;               // ccmi_mix: a mix-staged frame's filter output (flt_elems), with a radius or a solarize
};

struct DecodePlan {
    std::vector<FramePlan> fr;
    size_t cst = 0;        // bytes of the constant part
    size_t total = 0;      // workspace bytes
    size_t desc_off = 0;   // ArmStreamDesc[n * CCMI_MAX_GRIDS]
    size_t tail_off = 0;   // batched-tail argument tables, tail_cap bytes
    size_t tail_cap = 0;
    size_t status_off = 0; // one word per (frame, latent grid): the ARM kernels' CCMI_ARM_FLAG_* bits
    size_t lat_tab_off = 0; // latent-store sink / source: the pack / unpack job table, lat_tab_cap bytes
    size_t lat_tab_cap = 0;
    bool col = false;      // a frame has colour ops (DecFmt::col of every frame)
    std::vector<DecCol> cols; // col: every frame's ops (DecTailFrame::col points here); empty otherwise
    bool col_stat = false; // a frame has a contrast op: the accumulators are cleared before the tails run
    size_t col_off = 0;    // col: one 64-bit accumulator per frame (S_j of its contrast op)
    // ccmi_filter: every frame's DecFlt when a frame takes the stage (DecTailFrame::flt points here, NULL
    // for the frames that do not); n_flt of them do, and their tables, kFltTableBytes each, follow the
    // job table in the one host image
    std::vector<DecFlt> flts;
    int n_flt = 0;
    size_t flt_tab_off = 0;
    // ccmi_tone with an op in the call: every frame's DecTone (DecTailFrame::tone points here for the
    // staged frames); the staged frames' tables grow to dec_flt_table_bytes(true), and tone_acc_bytes
    // at tone_acc_off hold the accumulator blocks, cleared in stream before the tails run
    std::vector<DecTone> tones;
    size_t tone_acc_off = 0, tone_acc_bytes = 0;
    size_t flt_table_bytes() const { return dec_flt_table_bytes(!tones.empty()) * (size_t)n_flt; }
    // ccmi_mix with a frame that takes the stage: every frame's DecMix (DecTailFrame::mix points here for
    // the n_mix mix-staged frames, which all take the filter stage); their table, kMixTableBytes each,
    // follows the filter stage's in the one host image
    std::vector<DecMix> mixes;
    int n_mix = 0;
    size_t mix_tab_off = 0;
    size_t mix_table_bytes() const { return kMixTableBytes * (size_t)n_mix; }
    // ccmi_blend with a frame that has terms or is silent: every frame's DecBlend; the blend-staged frames
    // count among the n_mix mix-staged ones (mixes is then sized whether or not the call has a ccmi_mix), and
    // the blend table follows the mix table in the one host image
    std::vector<DecBlend> blends;
    size_t blend_tab_off = 0;
    size_t blend_table_bytes() const { return blends.empty() ? 0 : dec_blend_table_bytes(n_mix); }
#if defined(CCMI_ARM_STAMPS)
    size_t dbg_off = 0;
#endif
    size_t n_status() const { return fr.size() * CCMI_MAX_GRIDS; }
};

// Header parse, argument and region validation, output sizes (rq.sizes / geom / info are
// filled) and the workspace layout.  No weights are decoded and nothing touches the GPU.
int decode_plan(const DecodeRequest &rq, DecodePlan &pl);

// Layout of a latent store for the planned frames' streams at element type `type` (the
// contract in ccmi.h): fills h.s[i].type / off / bytes / ups_off / syn_off / grid_off and
// h.store_bytes (h.s sized here, the FrameHosts left alone).  Host arithmetic.
int latent_store_layout(const DecodePlan &pl, int type, ccmi_latents &h);

// For the calls that make a handle without a decode (dec_store_file.cpp): DecSynArgs::f24 of
// decoded synthesis integers, as the build computes it; and the thread's record of the last
// call (ARM flags and tail groups cleared, ccmi_decode_last_timing's four figures set).
bool dec_syn_weights_fit24(const FrameHost &f);
void dec_set_last_call(const float ms[4]);

} // namespace ccmi
