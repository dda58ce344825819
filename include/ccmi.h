/*
 * ccmi.h -- C ABI of libccmi, the MI355X (gfx950) implementation of Cool-chic's
 * per-image decode / forward hot path.
 *
 * Every entry point takes plain pointers and sizes (no C++ or torch types), is
 * reentrant (no globals; per-call state only) and never calls exit(): errors are
 * returned as a CCMI_ERR_* code with a message in ccmi_last_error() (thread-local).
 * Device pointers are caller-owned; kernels are enqueued on the caller's stream
 * (a hipStream_t passed as void*, e.g. torch.cuda.current_stream().cuda_stream).
 *
 * Two forms of the hot path, mirroring the reference:
 *   A. float forward  (coolchic/enc/component/coolchic.py:291-479): ARM probability
 *      model + rate, upsampling, synthesis, frame post-processing;
 *   B. fixed-point .cool bitstream decoder (coolchic/cpp/): CABAC + integer ARM,
 *      integer upsampling, integer synthesis, bit-exact with the reference C decoder.
 */
#ifndef CCMI_H
#define CCMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCMI_OK 0
#define CCMI_ERR_ARG 1         /* invalid argument / shape */
#define CCMI_ERR_HIP 2         /* HIP runtime error (no device, launch failure, ...) */
#define CCMI_ERR_UNSUPPORTED 3 /* architecture or stream feature not implemented */
#define CCMI_ERR_BITSTREAM 4   /* malformed .cool bitstream */
#define CCMI_ERR_IO 5          /* file open / read / write failure */

#define CCMI_MAX_GRIDS_PUBLIC 8
#define CCMI_MAX_SYN_LAYERS 16

/* Thread-local message for the last failing call on this thread. */
const char *ccmi_last_error(void);
/* ABI version (major*100 + minor). */
int ccmi_version(void);
/* Number of visible HIP devices (0 when none; never fails). */
int ccmi_device_count(void);

/* ------------------------------------------------------------------------- */
/* Path A: float forward, batched over independent frames of the same size and */
/* architecture.  Each frame has its own parameters (Cool-chic overfits one     */
/* network per image).  Latents of one frame are the flat concatenation of its  */
/* grids, grid l being h[l] x w[l] (coolchic.py:360-363).                        */
/* ------------------------------------------------------------------------- */

/* ARM: causal context gather + MLP + Laplace rate for every latent.
 * Replaces _get_neighbor (arm.py:308-352), Arm.forward (arm.py:227-268) and the
 * rate of CoolChicEncoder.forward (coolchic.py:395-424).
 * params per frame, float32: for each hidden layer l < n_hidden: W_l [d][d] (out,in)
 * then b_l [d]; then W_out [2][d], b_out [2]  (= arm.mlp state_dict order). */
typedef struct ccmi_arm_args {
    const float *latent;    /* [batch][latent_stride], N = sum h[l]*w[l] used; stride 0: shared */
    int64_t latent_stride;
    int n_grids;
    int h[CCMI_MAX_GRIDS_PUBLIC];
    int w[CCMI_MAX_GRIDS_PUBLIC];
    float gain;             /* encoder gain (coolchic.py:91) */
    int quantize;           /* 1: y = round(gain * latent) (eval quantizer); 0: latent used as is */
    int dim_arm;            /* 8, 16, 24 or 32 */
    int n_hidden;           /* 0..4 */
    const float *params;
    int64_t param_stride;
    float *mu;              /* optional outputs [batch][out_stride] (NULL to skip) */
    float *scale;
    float *log_scale;
    float *rate;            /* bits per latent, optional */
    int64_t out_stride;
    int batch;
} ccmi_arm_args;
int ccmi_arm_forward_f32(const ccmi_arm_args *args, void *stream);

/* The same call with the kernel form named.  Both forms give the same bits.
 *   CCMI_ARM_FORM_DEFAULT: the pairs form where it exists and a buffer is at hand, else the row form;
 *   CCMI_ARM_FORM_ROWS:    the row form (one output unit of two latents per packed register), reads
 *                          args->params directly; every dim_arm;
 *   CCMI_ARM_FORM_PAIRS:   the pairs form (two output units of one latent per packed register;
 *                          dim_arm 8 and 16), CCMI_ERR_UNSUPPORTED where it cannot run.
 * ccmi_arm_forward_f32 is the call with CCMI_ARM_FORM_DEFAULT.
 *
 * The pairs form reads a transposed copy of the parameters, written by one small launch on `stream`
 * ahead of the ARM kernel on every call (params may change between calls), into a device buffer the
 * library owns:
 *  - one buffer per (device, stream), grown on demand; calls on one stream are ordered by the
 *    stream, so they share it.  Two graphs captured on one stream share it too: replay them one
 *    after the other, not concurrently;
 *  - a buffer that was handed to a launch is neither freed nor moved before the library unloads (a
 *    captured graph may hold its address);
 *  - nothing is allocated while `stream` is capturing.  If the stream has no buffer of sufficient
 *    size by then, CCMI_ARM_FORM_DEFAULT runs the row form (CCMI_ARM_FORM_PAIRS fails): make one
 *    eager call of the same shape on the stream before capturing, as a capture needs anyway. */
#define CCMI_ARM_FORM_DEFAULT 0
#define CCMI_ARM_FORM_ROWS 1
#define CCMI_ARM_FORM_PAIRS 2
int ccmi_arm_forward_f32_form(const ccmi_arm_args *args, void *stream, int form);
/* The transposed copy of one frame's parameters, on the host (the permutation the device copy
 * applies): writes and returns the number of floats of the packed block, a multiple of 16; -1 on a
 * bad argument.  Layout: every row Wt[i][0..d) (the weights that multiply input i), then b[d], per
 * hidden layer, each row padded with zeros to 16 floats; then (W_out[0][i], W_out[1][i]) for
 * i < d, b_out[2], zeros. */
int ccmi_arm_pack_host(const float *params, int dim_arm, int n_hidden, float *out);
/* The tiles of a ccmi_arm_forward_f32 launch over `batch` frames of the grids h[], w[], on the
 * host, with the constants the kernels use: a workgroup owns 8 x 64 latents of one grid of one
 * frame; the tiles are numbered frame by frame, in a frame grid by grid, in a grid row by row.
 * Writes the launch's tile count to *n_tiles (may be NULL) and, for the tiles first .. first +
 * count - 1, (frame, grid, first row, first column) to out[4 * i ..].  CCMI_ERR_ARG for what the
 * launch itself refuses (a frame of more than 2^30 latents, 2^31 tiles or more) and for tiles
 * outside the launch. */
int ccmi_arm_tile_map(int n_grids, const int *h, const int *w, int batch, int64_t first, int count, int *out,
                      int64_t *n_tiles);

/* Standalone pieces of the ARM for API parity with the reference modules (the fused
 * ccmi_arm_forward_f32 is what CoolChicEncoder.forward uses):
 *  ccmi_arm_context_f32: _get_neighbor (arm.py:308-352), grids [batch][h][w] -> [batch][h*w][dim_arm]
 *  ccmi_arm_mlp_f32:     Arm.forward (arm.py:227-268) on given contexts [m][dim_arm] -> mu, scale,
 *                        log_scale [m] (any may be NULL); params as in ccmi_arm_args (one model). */
int ccmi_arm_context_f32(const float *grid, int batch, int h, int w, int dim_arm, float *out, void *stream);
int ccmi_arm_mlp_f32(const float *ctx, int64_t m, int dim_arm, int n_hidden, const float *params, float *mu,
                     float *scale, float *log_scale, void *stream);

/* Upsampling: Upsampling.forward in eval mode (upsampling.py:476-506, separable
 * paths :205-209 and :337-353).  params per frame, float32: n_ups kernels of ups_k
 * taps (full symmetric kernels, conv_transpose2ds[i]), then n_pre kernels of
 * pre_k taps (conv2ds[i]).  out: [batch][n_grids][H][W] with H,W = h[0],w[0]. */
typedef struct ccmi_ups_args {
    const float *latent;
    int64_t latent_stride;
    int n_grids;
    int h[CCMI_MAX_GRIDS_PUBLIC];
    int w[CCMI_MAX_GRIDS_PUBLIC];
    float gain;
    int quantize;
    int ups_k;              /* even, >= 4 */
    int n_ups;
    int pre_k;              /* odd */
    int n_pre;
    const float *params;
    int64_t param_stride;
    float *out;
    int64_t out_stride;
    void *workspace;        /* device scratch of ccmi_ups_workspace_bytes() */
    size_t workspace_bytes;
    int batch;
} ccmi_ups_args;
size_t ccmi_ups_workspace_bytes(int n_grids, const int *h, const int *w, int batch);
int ccmi_ups_forward_f32(const ccmi_ups_args *args, void *stream);
/* The same with the form of the pyramid chosen; every form gives the same bits in out.
 *   CCMI_UPS_FORM_DEFAULT: with ups_k = 8 and pre_k = 7, per step one launch of the row kernel (a
 *     workgroup makes one channel, or half of the refined latent, of a 32 x 128 destination tile
 *     with 128-bit stores); other tap counts run LEVELS;
 *   CCMI_UPS_FORM_LEVELS:  per step one launch with one channel of a 16 x 64 tile per workgroup.
 * Both write every level's stack to the workspace.
 * ccmi_ups_forward_f32 is the call with CCMI_UPS_FORM_DEFAULT. */
#define CCMI_UPS_FORM_DEFAULT 0
#define CCMI_UPS_FORM_LEVELS 1
int ccmi_ups_forward_f32_form(const ccmi_ups_args *args, void *stream, int form);

/* Synthesis: Synthesis.forward (synthesis.py:264-277, SynthesisConv2d :69-84):
 * conv layers with replicate padding, optional residual, optional ReLU.
 * params per frame, float32, per layer: W [n_out][c_in][ks][ks] then b [n_out]. */
typedef struct ccmi_syn_layer {
    int n_out;
    int ks;
    int residual;
    int relu;
} ccmi_syn_layer;

typedef struct ccmi_syn_args {
    const float *in;        /* [batch][c_in][h][w] */
    int64_t in_stride;
    int c_in;
    int h;
    int w;
    int n_layers;
    ccmi_syn_layer layers[CCMI_MAX_SYN_LAYERS];
    const float *params;
    int64_t param_stride;
    float *out;             /* [batch][n_out_last][h][w] */
    int64_t out_stride;
    void *workspace;        /* ccmi_syn_workspace_bytes(); may be NULL for fused architectures */
    size_t workspace_bytes;
    int batch;
} ccmi_syn_args;
size_t ccmi_syn_workspace_bytes(const ccmi_syn_args *args);
int ccmi_syn_forward_f32(const ccmi_syn_args *args, void *stream);

/* Frame post-processing of FrameEncoder.forward in eval mode (frame.py:175-183):
 * x -> clamp(round(x * (2^bitdepth-1)) / (2^bitdepth-1), 0, 1), optionally 444->420
 * nearest (yuv.py:275-299).  out420: Y [h][w] then U, V [h/2][w/2] per frame;
 * out444: [3][h][w] per frame. */
typedef struct ccmi_post_args {
    const float *in;        /* [batch][3][h][w] raw synthesis output */
    int64_t in_stride;
    int h;
    int w;
    int bitdepth;
    int yuv420;
    float *out;
    int64_t out_stride;
    int batch;
} ccmi_post_args;
int ccmi_post_f32(const ccmi_post_args *args, void *stream);

/* Fused decode tail: Upsampling.forward -> Synthesis.forward -> post-processing of
 * FrameEncoder.forward (eval) as ONE pass that never materialises the [n_grids][H][W]
 * upsampled stack nor the raw synthesis output (the composition of
 * ccmi_ups_forward_f32, ccmi_syn_forward_f32 and ccmi_post_f32, the decoder's path:
 * coolchic.py:395-437 then frame.py:175-183).  ups.out and syn.in are ignored;
 * syn.c_in must equal ups.n_grids and syn.h/w equal ups.h[0]/w[0]; ups.workspace as for
 * ccmi_ups_forward_f32.  bitdepth > 0: out receives the post-processed frame (layout
 * of ccmi_post_f32); bitdepth == 0: out receives the raw synthesis output.
 * CCMI_ERR_UNSUPPORTED when the architecture has no fused kernel (ups_k != 8,
 * pre_k != 7, or a synthesis outside the fused plan): run the three stages instead. */
typedef struct ccmi_decode_args {
    ccmi_ups_args ups;
    ccmi_syn_args syn;
    int bitdepth;
    int yuv420;
    float *out;
    int64_t out_stride;
    int stages;             /* 0 = all; bit 0: upsampling pyramid down to level 1 (into
                               ups.workspace), bit 1: the fused full-resolution kernel --
                               lets a caller time the two apart.  bit 3 (opt-in, the 7-grid
                               48-wide-head decoders): the fused kernel also evaluates the
                               level-2 -> 1 step and the pyramid stops at level 2 (same values
                               bit for bit; measured slower).  bit 4: the
                               fused kernel's runs hold one window each (cap 1 of
                               ccmi_fused_run_plan: every window pays the vertical halo; same
                               values bit for bit, for A/B runs and tests).  bit 5: the
                               pyramid in CCMI_UPS_FORM_LEVELS (same values bit for bit, for
                               A/B runs and tests) */
    int head;               /* synthesis 1x1 head arithmetic, CCMI_HEAD_*: both are fp32 (the
                               MFMA form's products are exact f32 fmas, summed in another
                               order); MFMA needs 7 inputs, 48 hidden units and >= 1 3x3 layer
                               and falls back to VALU otherwise; GENERIC is a test form: the
                               runtime-width VALU head without the unrolled 48-wide kernel's
                               scaled ReLU (bitwise equal to VALU while every hidden
                               pre-activation h has 2^-94 <= |h| <= 2^32 or h <= 0) */
} ccmi_decode_args;
enum { CCMI_HEAD_DEFAULT = 0, CCMI_HEAD_VALU = 1, CCMI_HEAD_MFMA = 2, CCMI_HEAD_GENERIC = 3 };
int ccmi_decode_forward_f32(const ccmi_decode_args *args, void *stream);

/* Host only (no device call): how the fused kernel splits the h rows of a frame into runs.
 * A workgroup walks a run of consecutive 32-row windows down a column strip; with n_sp 3x3
 * layers a run of n windows emits 32 n - 2 n_sp rows.  cap is the most windows a run may
 * hold (< 1: the library's built default; n_sp == 0: always 1).  Returns the number of runs
 * (-1 on a bad argument) and fills the first output row and the window count of the first
 * max_runs of them; run i ends where run i + 1 starts, the last one at h.  cap_used (may be
 * NULL) receives the cap applied. */
int ccmi_fused_run_plan(int h, int n_sp, int cap, int *start, int *windows, int max_runs, int *cap_used);

/* ------------------------------------------------------------------------- */
/* Path B: fixed-point .cool decoder, bit-exact with coolchic/cpp.             */
/* ------------------------------------------------------------------------- */

/* Same contract as the reference pybind cc_decode_cpu(in, out, bitdepth, chroma,
 * verbosity) (ccdecapi_cpu.cpp:20-30, ccdecapi.cpp:673-857): 0 on success, 1 on
 * failure; bitdepth/chroma 0 = take from the header; output format by extension
 * (.yuv -> planar 420/444, otherwise PPM).  Runs on HIP device `device`. */
int ccmi_decode_file(const char *in_path, const char *out_path, int out_bitdepth,
                     int out_chroma, int verbosity, int device);

/* Throughput entry point: decode n independent in-memory .cool streams (intra
 * frames) in one batched launch sequence.  out[i] receives the same bytes the
 * reference writes for stream i (YUV if as_yuv, else PPM), out_caps[i] its
 * capacity; out_sizes[i] (optional) the byte count written.  Host buffers. */
int ccmi_decode_batch(const uint8_t *const *streams, const size_t *lens, int n,
                      uint8_t *const *out, const size_t *out_caps, size_t *out_sizes,
                      int out_bitdepth, int out_chroma, int as_yuv, void *stream);

/* Device-side stage times (ms, HIP events on the decode stream) of this thread's last
 * successful ccmi_decode_batch / ccmi_decode_file: [0] upload of streams + weights,
 * [1] ARM + CABAC latent decode, [2] upsampling + synthesis + output conversion,
 * [3] download of the decoded bytes (0 after ccmi_decode_batch_dev: nothing is downloaded). */
int ccmi_decode_last_timing(float *ms4);

/* What the latent decode of this thread's last ccmi_decode_* call did, per stream: flags[i]
 * ORs the CCMI_ARM_FLAG_* bits of stream i's latent grids (*n = streams reported, at most
 * cap).  TIMEOUT is an error (the call itself returned CCMI_ERR_HIP and discarded the
 * output); the other bits say which integer multiply forms ran, i.e. which paths a stream
 * exercised (the reference's int32 ARM, arm_cpu.cpp:65-95, has one form).  The chain kernel's
 * wait limit is 2^24 polls, or the environment's CCMI_DEC_SPIN_CAP (a test hook: 0 makes
 * every wait give up at once).  Every decode call clears the record when it starts, so a
 * call that fails before its status words are read back reports no stream (*n = 0), not the
 * streams of the call before it. */
#define CCMI_ARM_FLAG_TIMEOUT 1u  /* a two-wave synchronisation wait gave up: decode invalid */
#define CCMI_ARM_FLAG_Q32 2u      /* chain kernel: a |q| > 16383 switched layer 0 to 32-bit products */
#define CCMI_ARM_FLAG_W32 4u      /* an ARM weight >= 2^23: every layer in 32-bit products */
#define CCMI_ARM_FLAG_PRE32 8u    /* chain helper wave: a chunk's contexts left 22 bits (32-bit sums) */
#define CCMI_ARM_FLAG_BIG 16u     /* spec / one-latent kernels: a |q| >= 2^15, layer 0 in 32-bit */
#define CCMI_ARM_FLAG_NARROW 32u  /* ccmi_latents_decode: a latent does not fit the store's element type */
int ccmi_decode_last_arm_flags(uint32_t *flags, int cap, int *n);

/* The integer latents of one intra stream (ARM + CABAC decode on the GPU; values, not
 * shifted), grids flattened in order: out needs sum_l h_l * w_l int32 (host buffer). */
int ccmi_decode_latents(const uint8_t *stream, size_t len, int32_t *out, size_t cap, void *stream_handle);

/* Row reductions for batched evaluation (quantize_model search, validation):
 * mode 0: out[b] = sum_i a[b][i];  mode 1: out[b] = sum_i (a[b][i] - t[b][i])^2, t_stride
 * 0 = one target for every row.  Accumulated in double.  Device pointers. */
int ccmi_row_reduce_f32(const float *a, int64_t a_stride, const float *t, int64_t t_stride, int64_t len, int batch,
                        int mode, double *out, void *stream);

/* ccmi_decode_batch with a caller-owned device workspace (no allocation inside):
 * ccmi_decode_batch_workspace_bytes() parses the streams' headers and returns the size the
 * same arguments need; the workspace must be 256-byte aligned.  ccmi_decode_batch_plan()
 * returns both the workspace size and every stream's output size (out_sizes[n]) from one
 * header-only pass (no CABAC, no GPU work).  Output buffers in pinned host memory make the
 * downloads real DMA copies that overlap the rest of the batch. */
int ccmi_decode_batch_workspace_bytes(const uint8_t *const *streams, const size_t *lens, int n,
                                      int out_bitdepth, int out_chroma, int as_yuv, size_t *bytes);
int ccmi_decode_batch_plan(const uint8_t *const *streams, const size_t *lens, int n, int out_bitdepth,
                           int out_chroma, int as_yuv, size_t *out_sizes, size_t *workspace_bytes);
int ccmi_decode_batch_ws(const uint8_t *const *streams, const size_t *lens, int n,
                         uint8_t *const *out, const size_t *out_caps, size_t *out_sizes,
                         int out_bitdepth, int out_chroma, int as_yuv, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Decoded frames as DEVICE tensors: the same decode as ccmi_decode_batch, but the samples
 * stay on the GPU in planar tensor layout (the layout of ccmi_post_f32 and of the trainer's
 * target): no frame data crosses PCIe, no file layout, no interleaving, no PPM header.
 *   444 output: [3][H][W] (RGB streams: planar R, G, B);
 *   420 output: Y[H][W], then U and V [H/2][W/2] (floor; the sample at the even row and
 *               column, as the .yuv writer takes it), one contiguous array of `elems` samples.
 * The sample values are exactly the integers the byte path writes for the same
 * (out_bitdepth, out_chroma); out_bitdepth 0 = the header's, any of 1..16 is accepted (the
 * .yuv writer's 8 / 10 limit is a file-format rule); out_chroma 0 = the header's, 420 or 444.
 *   CCMI_SAMPLE_U8:  uint8,  bitdepth <= 8 (else CCMI_ERR_ARG);
 *   CCMI_SAMPLE_U16: uint16, native byte order;
 *   CCMI_SAMPLE_F32: (float)sample / (float)(2^bitdepth - 1), one correctly rounded division.
 * ccmi_decode_batch_dev_plan() is the header-only pass (no CABAC, no GPU work): geometry of
 * every stream's output and the device workspace the same arguments need.
 * ccmi_decode_batch_dev(): out_dev[i] is a device pointer with room for out_caps[i] BYTES
 * (>= elems * sample size); it only needs the alignment of one sample (frames of a stacked
 * batch may start at any sample).  workspace NULL: the library allocates for the call;
 * otherwise >= workspace_bytes of the plan, 256-byte aligned.  The call synchronises
 * `stream` before it returns (the ARM status words are read back: a CCMI_ARM_FLAG_TIMEOUT is
 * CCMI_ERR_HIP), ccmi_decode_last_arm_flags() works as for the byte path and
 * ccmi_decode_last_timing() reports [3] (download) as 0. */
enum { CCMI_SAMPLE_U8 = 0, CCMI_SAMPLE_U16 = 1, CCMI_SAMPLE_F32 = 2 };
typedef struct ccmi_frame_geom {
    int width, height;
    int bitdepth;        /* of the output samples (out_bitdepth, or the header's) */
    int chroma;          /* 420 or 444, of the output */
    int frame_data_type; /* as in the stream header (0 rgb, 1 yuv420, 2 yuv444) */
    size_t elems;        /* samples per frame: 3 H W, or H W + 2 (H/2)(W/2) */
} ccmi_frame_geom;
int ccmi_decode_batch_dev_plan(const uint8_t *const *streams, const size_t *lens, int n,
                               int out_bitdepth, int out_chroma, int sample_type,
                               ccmi_frame_geom *geom /* [n] */, size_t *workspace_bytes);
int ccmi_decode_batch_dev(const uint8_t *const *streams, const size_t *lens, int n,
                          void *const *out_dev, const size_t *out_caps, int sample_type,
                          int out_bitdepth, int out_chroma, void *workspace,
                          size_t workspace_bytes, void *stream);

/* A region of interest of the same decode: roi[i] (luma samples, x / y = top-left corner) is
 * the window of stream i's frame that is decoded into out_dev[i]; roi NULL, or a rect of
 * 0, 0, W, H, is the whole frame, with the samples and the workspace size of
 * ccmi_decode_batch_dev / _plan.  geom[i].width / height are the rect's w / h and elems is
 * 3 w h (444) or w h + 2 (h/2)(w/2) (420).  The samples are, one for one, the crop of the
 * whole-frame decode:
 *   444 output: [3][h][w] = full[:, y:y+h, x:x+w];
 *   420 output: x and y must be even (else CCMI_ERR_ARG); Y = fullY[y:y+h, x:x+w], U and V =
 *               full[y/2 : y/2 + h/2, x/2 : x/2 + w/2] (an odd w or h drops the chroma of the
 *               last column or row, as an odd frame does).
 * w < 1, h < 1, x < 0, y < 0, x + w > W or y + h > H is CCMI_ERR_ARG (the message names the
 * stream) and nothing is written.  out_caps, the sample types, the one-sample alignment rule,
 * the stream synchronisation, ccmi_decode_last_timing() and ccmi_decode_last_arm_flags() are
 * those of ccmi_decode_batch_dev.
 * Streams with a fused synthesis (single branch; every reference architecture) decode the
 * window only (windowed = 1): the pyramid and the synthesis run on the windows the region
 * needs at each level, the workspace is sized by them, and the ARM + CABAC decode of latent
 * grid l stops after arm_rows[l] rows (the raster-order chain cannot skip rows above the
 * window or columns beside it).  The ARM flags then describe the rows that were decoded: a
 * wide-form latent below row arm_rows[l] is never seen.  Other streams run the whole-frame
 * tail and crop in the output kernel (windowed = 0, arm_rows[l] = h_l, whole-frame workspace).
 * Streams of one architecture, one frame size and one region size share their launches
 * whatever their origins. */
typedef struct ccmi_rect { int x, y, w, h; } ccmi_rect;
typedef struct ccmi_roi_info {
    int n_grids;
    int arm_rows[CCMI_MAX_GRIDS_PUBLIC]; /* latent rows of grid l the ARM + CABAC decode produces */
    int windowed;                        /* 1: the tail runs on windows; 0: whole-frame tail, cropped at the output stage */
} ccmi_roi_info;
int ccmi_decode_batch_dev_roi_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                   const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth,
                                   int out_chroma, int sample_type, ccmi_frame_geom *geom /* [n] */,
                                   ccmi_roi_info *info /* [n] or NULL */, size_t *workspace_bytes);
int ccmi_decode_batch_dev_roi(const uint8_t *const *streams, const size_t *lens, int n,
                              const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev,
                              const size_t *out_caps, int sample_type, int out_bitdepth,
                              int out_chroma, void *workspace, size_t workspace_bytes, void *stream);

/* Decode once, render often: a resident form of decoded streams.  The ARM + CABAC chain is
 * serial in raster order and its output, the integer latents, does not depend on the region,
 * the output bitdepth, the chroma format or the sample type.  ccmi_latents_decode() runs that
 * chain once and keeps the latents (packed to latent_type values) and the upsampling and
 * synthesis integers in a caller-owned device store; ccmi_latents_render() then produces any
 * region of any of the streams at the cost of the decoder tail alone.
 * THE SAMPLES ccmi_latents_render WRITES ARE, ONE FOR ONE, THOSE ccmi_decode_batch_dev_roi
 * WRITES FOR THE SAME STREAM, REGION AND OUTPUT ARGUMENTS.
 *
 * The handle is opaque and no global: it holds no lock, the render calls take it const, and
 * any number of threads may render from one handle (each with its own workspace and stream).
 * It lives on the host (parsed headers, decoded networks, the store's layout) and never refers
 * to `streams` or `workspace` after ccmi_latents_decode returns; the store memory stays the
 * caller's and must outlive the handle's last render.
 *
 * ccmi_latents_plan(): header-only (no CABAC, no GPU): bytes of the device store for these
 * streams at this element type (store_bytes_each[n] optional) and the workspace the build
 * needs.  Store layout: stream i starts 256-byte aligned at the sum of store_bytes_each[< i];
 * it holds the upsampling integers, the synthesis integers, then each latent grid's h_l * w_l
 * values, every part 16-byte aligned, and store_bytes_each[i] is its size rounded up to 256 (so
 * store_bytes is the sum).  A grid whose coded substream is empty takes no store bytes and
 * renders as zeros.  Per stream the store is at most 4 (ups + syn + blend ints) + N sizeof(T) +
 * 256 (n_grids + 4) bytes, N = the stream's latents.
 *
 * ccmi_latents_decode(): store = device memory, 256-byte aligned, >= store_bytes; workspace as
 * for ccmi_decode_batch_dev (NULL: allocated for the call).  A latent that does not fit the
 * element type (I8: -128..127, I16: -32768..32767) is never saturated or wrapped: the call
 * returns CCMI_ERR_UNSUPPORTED naming the first such stream, its grid and the type, creates no
 * handle, and ccmi_decode_last_arm_flags() shows CCMI_ARM_FLAG_NARROW for exactly the streams
 * that need a wider type.  The other ARM flags and TIMEOUT (CCMI_ERR_HIP) are reported as by
 * every decode.  store == NULL: no GPU call is made and the handle is plan-only
 * (ccmi_latents_render_plan works, ccmi_latents_render and ccmi_latents_values are
 * CCMI_ERR_ARG).  ccmi_decode_last_timing(): [1] the ARM + CABAC stage, [2] the pack.
 *
 * ccmi_latents_values(): stream i's latents as int32 values on the device, grids flattened in
 * order (the device counterpart of ccmi_decode_latents); cap_elems >= sum_l h_l * w_l.
 *
 * ccmi_latents_render_plan() / ccmi_latents_render(): m output frames; frame j is stream
 * index[j] of the handle (index NULL: m must equal the handle's count and frame j is stream j;
 * repeats and any order are allowed), region roi[j] (roi NULL, or a rect of 0, 0, W, H: the
 * whole frame).  geom, info, the sample types, out_caps, the one-sample alignment rule, the 420
 * even-origin rule and the error for a region outside the frame are those of
 * ccmi_decode_batch_dev_roi(_plan); info[j].arm_rows are the latent rows the tail's planes hold.
 * index[j] outside [0, count), m < 1, a NULL handle, and a plan-only handle passed to
 * ccmi_latents_render are CCMI_ERR_ARG, found before any HIP call, the message naming frame j.
 * The render workspace holds the tail's scratch and tables only: no coded bytes, no networks
 * (the tail reads them from the store), no ARM descriptors.  Both GPU calls synchronise
 * `stream` before they return.  The render calls run no ARM: they clear the ARM flag record
 * (ccmi_decode_last_arm_flags: *n = 0), and ccmi_decode_last_timing() after a render reports
 * [0] the table upload, [1] the unpack of the store into the tail's planes, [2] the tail, [3] 0. */
typedef struct ccmi_latents ccmi_latents;
enum { CCMI_LATENT_I8 = 0, CCMI_LATENT_I16 = 1, CCMI_LATENT_I32 = 2, CCMI_LATENT_SEG = 3 /* by compaction only */ };
int ccmi_latents_plan(const uint8_t *const *streams, const size_t *lens, int n, int latent_type,
                      size_t *store_bytes, size_t *store_bytes_each /* [n] or NULL */, size_t *workspace_bytes);
int ccmi_latents_decode(const uint8_t *const *streams, const size_t *lens, int n, int latent_type,
                        void *store, size_t store_bytes, void *workspace, size_t workspace_bytes,
                        void *stream, ccmi_latents **out);
void ccmi_latents_free(ccmi_latents *h); /* host side only; NULL is a no-op */
int ccmi_latents_count(const ccmi_latents *h);
int ccmi_latents_values(const ccmi_latents *h, int i, int32_t *out_dev, size_t cap_elems, void *stream);
int ccmi_latents_render_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                             const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                             int sample_type, ccmi_frame_geom *geom /* [m] */, ccmi_roi_info *info /* [m] or NULL */,
                             size_t *workspace_bytes);
int ccmi_latents_render(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                        const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                        int sample_type, int out_bitdepth, int out_chroma, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Compact stores and one handle over many stores.
 *
 * CCMI_LATENT_SEG: per-segment bit widths.  A stream's part of the store is laid out as for the
 * other types (256-byte aligned; upsampling integers, synthesis integers, then the grids; every
 * part 16-byte aligned; the size rounded up to 256; an empty grid takes no bytes and renders as
 * zeros); only the form of a non-empty grid l (h_l x w_l) differs: a descriptor table, then a
 * payload, each 16-byte aligned.
 *   Segments: nseg = ceil(w_l / 64); segment (r, s) covers columns [64 s, min(64 s + 64, w_l)) of
 *   row r: c values.
 *   Width code k in 0..5 stands for b = 0, 2, 4, 8, 16, 32 bits; a segment's k is the smallest
 *   code with every value in [-2^(b-1), 2^(b-1) - 1]; b = 0: every value is 0.
 *   Payload: segment (r, s) takes ceil(c b / 32) 32-bit words; segments follow each other in
 *   (r, s) row-major order without gaps, off(r, s) = the words before it.  Value j is the two's-
 *   complement field at bits [j b, (j + 1) b) of the segment's words read as one little-endian bit
 *   string (bit t is bit t % 32 of word t / 32); the last word's trailing bits are 0.
 *   Descriptors: desc[r nseg + s] = (off << 3) | k, uint32, h_l nseg of them.  off must fit 29
 *   bits: a grid where it does not is CCMI_ERR_UNSUPPORTED naming stream and grid.
 * The form is a function of the latents alone: compactions of the same streams from I8, I16 and
 * I32 stores give the same descriptor tables and payloads, byte for byte.
 *
 * A SEG store has a data-dependent size, so it is not built from coded streams
 * (ccmi_latents_plan / ccmi_latents_decode with CCMI_LATENT_SEG: CCMI_ERR_ARG) but from a built
 * I8 / I16 / I32 handle, which may be freed afterwards with its store:
 * ccmi_latents_compact_plan(): host arithmetic, works on a plan-only handle too: the size of the
 *   compact store if every segment took 32 bits, and the workspace of the two calls below.
 * ccmi_latents_compact_measure(): the width pass and the offset scan on the GPU; the exact store
 *   size and (optional) the per-stream sizes, 256-byte multiples whose sum it is.
 * ccmi_latents_compact(): stateless (derives the widths again), writes the store (device, 256-byte
 *   aligned) and creates the handle.  store_bytes below the exact size: CCMI_ERR_ARG naming the
 *   size needed, nothing written to `store`, no handle.
 * workspace NULL: allocated for the call.  The new handle never refers to src, its store or the
 * workspace.  Both GPU calls synchronise `stream` before they return.  A NULL src, a plan-only src
 * where the GPU is needed, and a src with a CCMI_LATENT_SEG stream are CCMI_ERR_ARG before any
 * HIP call.
 *
 * ccmi_latents_concat(): host only.  The new handle's streams are those of parts[0], then
 * parts[1], ..., each with its own type (I8 / I16 / I32 / SEG may mix) and its own device
 * location.  The parts may be freed afterwards; their store memory stays the caller's and must
 * outlive the new handle's last render.  Plan-only parts give a plan-only handle; mixing plan-only
 * and resident parts, n_parts < 1, a NULL entry and more than INT_MAX streams are CCMI_ERR_ARG.
 * Every ccmi_latents_render* call, its plan and ccmi_latents_values take such a handle: frames
 * are planned and grouped exactly as if the streams sat in one store
 * (ccmi_decode_last_tail_groups reports the same counts), the run launches one unpack per
 * storage type present, and render plans and workspaces do not depend on the storage type.
 * ccmi_latents_stream_info(): stream i's CCMI_LATENT_* type and its bytes in its store (either
 * pointer may be NULL).
 * Measured (profiles/decode_compact_ab.txt): 274 kB per 720p stream against 2.21 MB at int16, 934 kB
 * per 1080p stream against 5.53 MB; 960 class-E streams measure in 12.5 ms and compact in 25 ms;
 * the 256 x 256 render_model call takes 11.0-11.2 ms from the int16 store, its compaction and a
 * concat of 8 compacted chunks alike (the unpack 0.28-0.29 ms against 0.27 ms). */
int ccmi_latents_compact_plan(const ccmi_latents *src, size_t *store_bytes_max, size_t *workspace_bytes);
int ccmi_latents_compact_measure(const ccmi_latents *src, void *workspace, size_t workspace_bytes, void *stream,
                                 size_t *store_bytes, size_t *store_bytes_each /* [count] or NULL */);
int ccmi_latents_compact(const ccmi_latents *src, void *store, size_t store_bytes, void *workspace,
                         size_t workspace_bytes, void *stream, ccmi_latents **out);
int ccmi_latents_concat(const ccmi_latents *const *parts, int n_parts, ccmi_latents **out);
int ccmi_latents_stream_info(const ccmi_latents *h, int i, int *latent_type, size_t *store_bytes);

/* Latent stores as files: export of any resident handle, verified import.
 *
 * THE FILE FORM.  Everything is little-endian.
 *   FILE = HEAD (64 bytes) | INDEX | zero padding to a multiple of 256 | DATA;  META = HEAD | INDEX.
 * HEAD: bytes 0-7 the magic "CCMILAT1"; 8 u32 version = 1; 12 u32 n_streams >= 1; 16 u64 index_bytes;
 *   24 u64 data_off = (64 + index_bytes) rounded up to 256; 32 u64 data_bytes; 40 u64[2] index_sum (the
 *   checksum below over the INDEX bytes); 56 u64 0.
 * INDEX: one record per stream, each a multiple of 8 bytes (one zero u32 of padding where needed),
 *   the fields in this order:
 *     u32 record_bytes; u32 latent_type (CCMI_LATENT_*); u64 part_bytes (this stream's part of DATA, a
 *     multiple of 256); u64[2] part_sum (the checksum over the part); u32 user_flags;
 *     14 i32: h, w, bitdepth, frame_data_type, intra_period, dim_arm, n_hidden, n_ups, ups_ks, n_pre,
 *       pre_ks, n_branches, sig_blk, n_layers (the .cool header's fields; n_layers = the latent grids);
 *     u32 the count of synthesis layers, then per layer 4 i32: n_out, ks, residual, relu;
 *     per grid u32 lat_n (the grid's coded bytes in its .cool stream; 0: an empty grid);
 *     per grid u32 seg_words: the grid's payload words of a CCMI_LATENT_SEG stream; 0 for the other
 *       types and for an empty grid;
 *     u32 the count of blend integers (n_branches if n_branches > 1, else 0), then the integers (i32).
 *   The upsampling and synthesis integers are not in the INDEX: a reader takes them from DATA.
 * DATA: the streams' parts one behind the other, stream i's at data_off + the part_bytes before it.
 *   A part is, byte for byte, the stream's part of a store of its type as defined above (upsampling
 *   integers: n_ups ups_ks + n_pre pre_ks int32; synthesis integers: per branch and layer n_out c_in
 *   ks ks + n_out int32, c_in = n_layers for the first layer, else the layer before's n_out; then the
 *   non-empty grids; every part 16-byte aligned; SEG: descriptor table, then seg_words payload words;
 *   the size rounded up to 256), and every byte the store contract leaves undefined (alignment
 *   padding, the tail) is 0.  No offset inside a part is stored: writer and reader derive the layout
 *   from the record, and part_bytes must equal the derived size.
 * Checksum of a byte range read as u32 words w_0 .. w_(n-1) (a range that is no multiple of 4 bytes
 *   zero-extended): sum[0] = sum of w_i, sum[1] = sum of (i + 1) w_i, both mod 2^64.  It guards
 *   against accidental corruption; memory safety does not rest on it.
 * A file is a function of the latents, the networks and the header facts alone: exports of the same
 * streams are identical byte for byte whatever sat in the stores' padding and whichever of I8 / I16 /
 * I32 a SEG store was compacted from.
 *
 * ccmi_latents_file_head(): the head's checks alone; meta_bytes = 64 + index_bytes, file_bytes =
 *   data_off + data_bytes (any of the three outputs may be NULL).
 * ccmi_latents_export_plan(): host arithmetic, works on a plan-only handle.  The file holds streams
 *   index[0..m) of the handle (NULL: every stream in order, m = the count; repeats and any order are
 *   allowed, so a file can be a re-sharding of a handle).
 * ccmi_latents_export(): any resident handle, a concat of mixed types over several stores included;
 *   a plan-only handle is CCMI_ERR_ARG before any HIP call.  `file` is host memory of file_bytes;
 *   workspace (device, 256-byte aligned; NULL: allocated for the call) holds the DATA image, which is
 *   cleared, gathered and checksummed on the device and downloaded in one copy.  The handle and its
 *   stores are only read: renders may run from them meanwhile.  user_flags[j] travels with stream j.
 * ccmi_latents_import_plan(): validates META; for streams [first, first + count) (count < 0: to the
 *   end) the range FILE[data_off, data_off + data_bytes) that holds their parts, their store bytes
 *   (store_bytes_each[i] = part_bytes; the store takes data_bytes) and the import's workspace.
 * ccmi_latents_import(): store == NULL and data == NULL: no HIP call, a plan-only handle from META
 *   alone (its networks' integers are zeros).  Otherwise: META is validated on the host; `data` (host)
 *   is copied to `store` (device, 256-byte aligned), which then is that DATA range byte for byte; the
 *   parts' checksums are taken on the device; every descriptor table of a SEG stream is verified on
 *   the device: every width code <= 5, every offset the exclusive prefix sum of the word counts of
 *   the segments before it, the total equal to seg_words.  After that off + words <= seg_words holds
 *   for every segment, so no render can read outside a grid's payload whatever the file held.  (That
 *   a code is the smallest that fits and that trailing bits are 0 is not checked: neither affects
 *   safety, only whether a re-export is canonical.)  The upsampling and synthesis integers are read
 *   from `data`.  Only then the handle is created.  The call writes exactly data_bytes of `store`,
 *   synchronises `stream`, clears the ARM flag record and the tail groups;
 *   ccmi_decode_last_timing() reports [0] the upload, [1] checksums + verify.
 *   Errors create no handle and name the stream (and grid).  CCMI_ERR_BITSTREAM: a malformed or
 *   inconsistent META (every header field is held to the .cool header's limits; a stream's upsampling
 *   and synthesis integers may number 2^22 at most; seg_words <= min(h_l w_l, 2^29 + 63)), a checksum
 *   mismatch, a descriptor fault.  CCMI_ERR_ARG, before any HIP call: a NULL pointer, first / count
 *   outside the file, data_bytes or store_bytes too short, a store not 256-byte aligned, a workspace
 *   too small or misaligned, store and data not both NULL or both set. */
int ccmi_latents_file_head(const void *head, size_t head_bytes /* >= 64 */, int *n_streams, size_t *meta_bytes,
                           size_t *file_bytes);
int ccmi_latents_export_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m, size_t *meta_bytes,
                             size_t *file_bytes, size_t *workspace_bytes);
int ccmi_latents_export(const ccmi_latents *h, const int *index, int m, const uint32_t *user_flags /* [m] or NULL */,
                        void *file /* host */, size_t file_bytes, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_import_plan(const void *meta, size_t meta_bytes, int first, int count /* < 0: to the end */,
                             size_t *data_off, size_t *data_bytes, size_t *store_bytes_each /* [count] or NULL */,
                             size_t *workspace_bytes);
int ccmi_latents_import(const void *meta, size_t meta_bytes, int first, int count,
                        const void *data /* host: FILE[data_off, data_off + data_bytes) of import_plan */, size_t data_bytes,
                        void *store, size_t store_bytes, void *workspace, size_t workspace_bytes, void *stream,
                        uint32_t *user_flags /* [count] or NULL */, ccmi_latents **out);

/* Formatted output: the same decode (coded streams, or a latent store) written as the tensor a
 * model or a display takes -- three full-size channels, optionally RGB, normalised, fp16 / bf16,
 * any strides (NCHW, NHWC, a view into the caller's canvas), optionally mirrored -- by one
 * output kernel that replaces the tensor output kernel: no float32 frame is staged and no extra
 * pass runs.  For output frame j, region pixel (y, x), channel c:
 *   1. s_0..s_2: the integer samples of the tensor path at (out_bitdepth, out_chroma).  444: all
 *      planes at (y, x).  420: plane 0 at (y, x), planes 1 and 2 the 420 plane's sample
 *      (y >> 1, x >> 1), i.e. the nearest-neighbour x2 upsample; the region's x, y, w AND h must
 *      be even (a whole frame too), else CCMI_ERR_ARG -- ask for out_chroma = 444 instead;
 *   2. p_k = (float)s_k / (float)(2^bitdepth - 1), one correctly rounded division (CCMI_SAMPLE_F32);
 *   3. CCMI_COLOUR_ASIS, or an RGB stream (frame_data_type 0): q = p.  CCMI_COLOUR_RGB on a YUV
 *      stream: q_c = clamp(((p_0 + a_c p_1) + b_c p_2) + o_c, 0, 1), every product and sum one
 *      float32 operation in this order; (a_c, b_c) are the float32 roundings of the BT.709-style
 *      matrix the reference's yuv2rgb uses and o_c of its offset / 255;
 *   4. r_c = q_c * scale[c] + bias[c], two float32 operations (no fused multiply-add);
 *   5. r_c to `elem`, round to nearest even;
 *   6. stored at out_dev[j] + c stride_c + y stride_y + x' stride_x (elements), x' = w - 1 - x
 *      when mirror[j] is non-zero, else x.
 * Strides all 0 mean planar contiguous (w h, w, 1).  Checked by the plan, before any GPU work,
 * CCMI_ERR_ARG naming the frame and nothing written: an unknown elem / colour, a non-finite scale
 * or bias, a negative stride, strides that let two elements of a frame share an address (sorted
 * by stride, each must be >= the previous stride times the previous extent), out_caps[j] below
 * (2 stride_c + (h - 1) stride_y + (w - 1) stride_x + 1) sizeof(elem), out_dev[j] not aligned to
 * one element, and the 420 evenness rule.  geom[j].width / height are the region's, elems is
 * 3 w h, chroma the format the samples were taken at.  The workspace is that of the same call
 * with CCMI_SAMPLE_F32.  Everything else (roi, index, info, workspace, the stream
 * synchronisation, timing and ARM flags) is as for ccmi_decode_batch_dev_roi(_plan) and
 * ccmi_latents_render(_plan), whose argument lists these follow with fmt in place of sample_type.
 * With unit stride_x (NCHW) or stride_c = 1, stride_x = 3 (NHWC) the kernel writes packed 8 / 16
 * byte stores wherever the destination is aligned; other strides take one store per element.
 * Measured (profiles/decode_model_ab.txt): 960 class-E streams from a latent store, 256 x 256
 * regions, RGB, ImageNet mean / std, bf16, NCHW: 11.1 ms per call (tail 8.2 ms) against 13.5 ms
 * for the CCMI_SAMPLE_F32 render (tail 8.0 ms) followed by the same steps as torch operations,
 * equal in every element; peak allocation above store and workspace 360 MiB against 3720 MiB. */
enum { CCMI_ELEM_F32 = 0, CCMI_ELEM_F16 = 1, CCMI_ELEM_BF16 = 2 };
enum { CCMI_COLOUR_ASIS = 0, CCMI_COLOUR_RGB = 1 };
typedef struct ccmi_tensor_fmt {
    int elem, colour;
    float scale[3], bias[3];
    int64_t stride_c, stride_y, stride_x; /* elements; all 0 = planar contiguous [3][h][w] */
    const uint8_t *mirror;                /* host, [n] or NULL */
} ccmi_tensor_fmt;
int ccmi_decode_batch_dev_fmt_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                   const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth,
                                   int out_chroma, const ccmi_tensor_fmt *fmt, ccmi_frame_geom *geom /* [n] */,
                                   ccmi_roi_info *info /* [n] or NULL */, size_t *workspace_bytes);
int ccmi_decode_batch_dev_fmt(const uint8_t *const *streams, const size_t *lens, int n,
                              const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev,
                              const size_t *out_caps, const ccmi_tensor_fmt *fmt, int out_bitdepth,
                              int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_fmt_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                 const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                 const ccmi_tensor_fmt *fmt, ccmi_frame_geom *geom /* [m] */,
                                 ccmi_roi_info *info /* [m] or NULL */, size_t *workspace_bytes);
int ccmi_latents_render_fmt(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                            const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                            const ccmi_tensor_fmt *fmt, int out_bitdepth, int out_chroma, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Resampled formatted output: the formatted sink with an output size.  Every frame's region, of
 * any size, is resampled to out_h x out_w by an antialiased triangle filter -- the filter of
 * interpolate(mode="bilinear", antialias=True, align_corners=False) and of PIL's BILINEAR --
 * between steps 3 and 4 of the ccmi_tensor_fmt contract, in the decoder's output stage: crop,
 * resize, colour, normalisation, element type, layout and mirror in one call, and frames of
 * different region sizes share the tail's launches.  rs == NULL is the _fmt call itself.
 * Steps 1-3 give q_c(y, x) over the region, h x w.  Then
 *   3a. weights, per axis: region extent I, output extent O, D = max(I, O).  For output index i
 *       and source index j in [0, I): u(i, j) = max(0, 2 D - |(2 j + 1) O - (2 i + 1) I|), an
 *       integer.  The taps of i are the j with u > 0, a contiguous run, clipped to the REGION (the
 *       region is the image being resized: the result equals crop-then-resize).  U(i) = sum_j
 *       u(i, j); w(i, j) = (float)u / (float)U, conversions to nearest even, one correctly
 *       rounded float32 division.  With I == O the only tap is j = i with w = 1: that pass is the
 *       identity, bit for bit;
 *   3b. horizontal pass, per region row y: t_c(y, i) = sum_j w_x(i, j) q_c(y, j), evaluated from 0
 *       over j ascending, every product and every sum its own float32 operation (no fused
 *       multiply-add);
 *   3c. vertical pass: r'_c(i, k) = sum_y w_y(i, y) t_c(y, k), evaluated the same way over y
 *       ascending.
 * Steps 4-6 apply to r' at the output size; the mirror is x' = out_w - 1 - x.
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame and nothing written:
 * out_w or out_h outside [1, 16384], a region side above 16384 (the weights' integers then fit
 * 32 bits), an unknown filter.  The strides, their aliasing check and out_caps refer to the
 * out_h x out_w frame; geom[j].width / height are out_w / out_h and elems is 3 out_w out_h.  The
 * 420 rule stays on the region (x, y, w and h even); the output size may be anything.
 * ccmi_roi_info is unchanged.  The workspace grows by the float32 intermediate t, [3][h][out_w]
 * per frame.  Streams with a fused synthesis of one architecture share one batched tail whatever
 * their region sizes (whole-frame requests: one per frame size, as ever); the others run their
 * per-frame tail.  ccmi_decode_last_tail_groups(): how many batched tail groups and how many
 * per-frame tails this thread's last decode or render call launched (0, 0 after a call that
 * failed or only planned, and after ccmi_latents_decode, which runs no tail).
 *
 * CCMI_FILTER_CUBIC: the same call with the Keys cubic, a = -0.5, in place of the triangle -- the
 * filter of interpolate(mode="bicubic", antialias=True, align_corners=False) and of PIL's BICUBIC,
 * its support scaled by max(I / O, 1).  filter is one value per call: 0 (triangle), 2 (cubic) or
 * 0x102 (cubic | CCMI_FILTER_CLAMP); 1 is reserved, and every other value is an unknown filter.
 * Steps 3b and 3c are the triangle's (the same two passes, taps ascending, sums from 0, the region
 * as the image); only the weights of 3a differ, and they stay integers:
 *   3a. per axis: D2 = 2 max(I, O), n(i, j) = |(2 j + 1) O - (2 i + 1) I|, in 64-bit arithmetic
 *         n < D2:         u = 3 n^3 - 5 n^2 D2 + 2 D2^3
 *         D2 <= n < 2 D2: u = -n^3 + 5 n^2 D2 - 8 n D2^2 + 4 D2^3   (negative: the side lobes)
 *       The taps of i are the j with n < 2 D2, a contiguous run, clipped to the region (a tap may
 *       have u = 0).  U(i) = sum_j u(i, j) > 0; w(i, j) = (float)u / (float)U: two int64 -> float32
 *       conversions to nearest even, one correctly rounded float32 division.  With I, O <= 16384
 *       every term stays below 2^51 and |U| below 2^61.  With I == O the neighbours' u is exactly 0
 *       and w(i, i) = 1: that pass is the identity, bit for bit.
 * The weights of a tap row sum to 1 but are not all positive, so r' may leave [0, 1] (torch's float
 * path does not clamp either).  With CCMI_FILTER_CLAMP, r' = min(max(r', 0), 1) after step 3c and
 * before the colour ops (step 3z) -- what a uint8 / PIL pipeline gives.  The flag is valid with
 * CCMI_FILTER_CUBIC only.  The workspace formula is unchanged.
 * Kernels (dec_out.hip): dec_resize_h<true>, dec_resize_h_batch<true> and the geometry Resize<true> of
 * dec_fmt, dec_fmt_col and dec_fmt_stat, the weights recomputed per thread by Horner in int64. */
enum { CCMI_FILTER_TRIANGLE = 0, CCMI_FILTER_CUBIC = 2, CCMI_FILTER_CLAMP = 0x100 };
typedef struct ccmi_resample { int out_w, out_h, filter; } ccmi_resample;
int ccmi_decode_batch_dev_rs_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                  const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth, int out_chroma,
                                  const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                  ccmi_frame_geom *geom /* [n] */, ccmi_roi_info *info /* [n] or NULL */,
                                  size_t *workspace_bytes);
int ccmi_decode_batch_dev_rs(const uint8_t *const *streams, const size_t *lens, int n,
                             const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev, const size_t *out_caps,
                             const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */, int out_bitdepth,
                             int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_rs_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                ccmi_frame_geom *geom /* [m] */, ccmi_roi_info *info /* [m] or NULL */,
                                size_t *workspace_bytes);
int ccmi_latents_render_rs(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                           const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                           const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */, int out_bitdepth,
                           int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_decode_last_tail_groups(int *batched, int *per_frame);

/* Warped formatted output: the formatted sink with an output size and one 2 x 3 matrix per frame.
 * Every output frame is out_h x out_w and every output pixel a bilinear sample of the decoded
 * frame at the position the frame's matrix gives -- rotation, scale, shear, translation, flip:
 * grid_sample(mode="bilinear", align_corners=False) with the grid in pixels -- between steps 3 and
 * 4 of the ccmi_tensor_fmt contract, in the decoder's output stage.  There is no roi: steps 1-3
 * define q_c(y, x) over the WHOLE frame, H x W, and the library derives the window of the frame it
 * has to decode.  For output row i, column k, every product, sum and difference one float32
 * operation in the order written (no fused multiply-add):
 *   3a. cx = (float)k + 0.5f, cy = (float)i + 0.5f;
 *       xs = ((m00 cx) + (m01 cy)) + m02, ys = ((m10 cx) + (m11 cy)) + m12: frame coordinates in
 *       pixels, pixel (y, x) covering [x, x + 1) x [y, y + 1);
 *   3b. u = xs - 0.5f, x0 = floor(u), fx = u - (float)x0; v, y0, fy alike from ys;
 *   3c. tap T_c(a, b), a, b in {0, 1}: q_c(y0 + a, x0 + b) where that lies in [0, H) x [0, W);
 *       otherwise fill[c] (CCMI_PAD_FILL), or q_c at the indices clamped to the frame
 *       (CCMI_PAD_EDGE);
 *   3d. top = (T(0,0) (1 - fx)) + (T(0,1) fx), bot alike from T(1, .), r' = (top (1 - fy)) + (bot fy).
 * Steps 4-6 apply to r' at the output size; mirror[j] is x' = out_w - 1 - x, as with a resample.
 * So an integer translation (m = 1 0 x / 0 1 y) is the crop at (x, y) bit for bit, and m00 = -1 a
 * flip, bit for bit.  There is no antialiasing (this is grid_sample, not
 * interpolate(antialias=True)): pure downscaling belongs to ccmi_resample.
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame and nothing written: warp
 * or matrix NULL, out_w or out_h outside [1, 16384], an unknown pad, a non-finite matrix entry or
 * fill, |m00| out_w + |m01| out_h + |m02| > 2^22 or the same sum of the second row (the bound on
 * every float32 intermediate: the position is then within 3 2^-24 2^22 = 0.75 pixel of exact
 * arithmetic and x0 fits an int), and a 420 sample format on a frame with an odd size.  The
 * strides, their aliasing check and out_caps refer to the out_h x out_w frame; geom[j].width /
 * height are out_w / out_h and elems is 3 out_w out_h.
 * window[j] (the _plan calls, optional) is the rectangle of the frame the tail renders for frame
 * j, computed in double from the float32 matrix: xs, ys at the four corner pixel centres (the map
 * is linear: the extremes); columns floor(min xs - 0.5) - 1 .. floor(max xs - 0.5) + 2 and rows
 * alike -- the taps' bounding box grown by one pixel for the float32 rounding --, each end CLAMPED
 * into the frame (never empty; it holds the edge pixels CCMI_PAD_EDGE needs even when the whole
 * output lies outside the frame), grown to even x, y, w, h for a 420 sample format.  It is a
 * superset of the in-frame taps and no part of the bitwise contract.  The workspace is that of the
 * _fmt call with roi = window (no intermediate); a window equal to the frame runs the whole-frame
 * tail, a stream without a fused synthesis its per-frame tail on the whole frame.  Streams with a
 * fused synthesis of one architecture share one batched tail whatever their matrices.  The
 * argument lists follow the _rs calls without roi; everything else (index, info, the stream
 * synchronisation, timing, ARM flags, ccmi_decode_last_tail_groups) is as for them.
 * Measured (profiles/decode_warp_ab.txt): 960 class-E streams from an int16 store, rotation +-30
 * degrees, scale 0.5-1.5, random centres, 224 x 224 bf16 RGB normalised: 14.8-14.9 ms per call (tail
 * 11.3 ms) in one tail group, against 194-209 ms for the CCMI_ELEM_F32 render of the same windows per
 * window size (737 groups) followed by torch's grid_sample; workspace 6.6 GiB.
 *
 * CCMI_WARP_CUBIC, or'ed into pad: every output pixel is a bicubic sample instead -- cubic
 * convolution with A = -0.75, grid_sample(mode="bicubic", align_corners=False).  pad is one value
 * per call: 0, 1, 0x100, 0x101 and, with CCMI_WARP_CLAMP (valid with CCMI_WARP_CUBIC only), 0x300
 * and 0x301; every other value is an unknown pad.  The struct is unchanged.  Steps 3a-3b are as
 * above; then, every product, sum and difference one float32 operation in the order written:
 *   3c. 16 taps T_c(a, b) = q_c(y0 - 1 + a, x0 - 1 + b), a, b in 0 .. 3, each with the fill / edge
 *       rule of the bilinear tap;
 *   3d. c_in(t) = ((((A + 2) t) - (A + 3)) t) t + 1, c_out(s) = ((((A s) - 5 A) s + 8 A) s) - 4 A
 *       with the constants A + 2 = 1.25, A + 3 = 2.25, 5 A = -3.75, 8 A = -6, 4 A = -3;
 *       gx = 1 - fx; wx = { c_out(fx + 1), c_in(fx), c_in(gx), c_out(gx + 1) }, wy alike from fy;
 *       row_a = sum_b T(a, b) wx[b], from 0 over b ascending; r' = sum_a row_a wy[a], from 0 over
 *       a ascending.
 * At fx = 0 the coefficients are exactly 0, 1, 0, 0, so an integer translation is still the crop
 * and m00 = -1 the flip, bit for bit.  r' may leave [0, 1]; with CCMI_WARP_CLAMP r' = min(max(r',
 * 0), 1) before the colour ops -- on r' whatever its taps were, fill included.
 * window[j] grows by one tap on each side: columns floor(min xs - 0.5) - 2 .. floor(max xs - 0.5)
 * + 3 and rows alike, then the same clamp into the frame and the same even-ing.
 * Kernels (dec_out.hip): the geometry Warp<true, false> of dec_fmt, dec_fmt_col and dec_fmt_stat.
 *
 * CCMI_WARP_PROJECTIVE (0x800; 0x400 stays an unknown pad), or'ed into pad: the frame's matrix is a
 * 3 x 3 homography, matrix is host [n][9], row-major m00 .. m22 of frame j, and the position is the
 * projective one -- torchvision's F.perspective convention: base grid at k + 0.5,
 * grid_sample(align_corners=False).  The struct is unchanged, so every entry point that takes a
 * ccmi_warp (_warp, _col, _flt, _tone, the decode and ccmi_latents_render_* forms, their _plan calls)
 * takes the flag.  pad is one value per call -- today's six plus 0x800, 0x801, 0x900, 0x901, 0xB00,
 * 0xB01; 0xA00 / 0xA01 (clamp without cubic) and everything else remain an unknown pad -- so a call
 * is wholly affine or wholly projective: a caller mixing both passes rows 0 0 1.  Step 3a becomes,
 * every product, sum and difference one float32 operation in the order written (no fused
 * multiply-add):
 *   3a'. cx = (float)k + 0.5f, cy = (float)i + 0.5f   (mirror as above: k -> out_w - 1 - k)
 *        xn = ((m00 cx) + (m01 cy)) + m02
 *        yn = ((m10 cx) + (m11 cy)) + m12
 *        wn = ((m20 cx) + (m21 cy)) + m22
 *        xs = xn / wn, ys = yn / wn: the correctly rounded IEEE float32 quotient (no
 *        reciprocal-multiply, no fast division).
 * Steps 3b-3d (bilinear, CCMI_WARP_CUBIC, CCMI_WARP_CLAMP, the fill / edge rule) and 4-6 are
 * unchanged.  With m20 = m21 = 0, m22 = 1, wn is exactly 1 and the quotient exact: the result equals
 * the 6-entry call's bit for bit, so an integer translation is still the crop and m00 = -1 the flip.
 * Checked by the plan, as above (CCMI_ERR_ARG naming the frame, before any GPU work, nothing
 * written), in double from the float32 entries.  With eps = 2^-24, S_r = |m_r0| out_w + |m_r1| out_h
 * + |m_r2| for r = 0, 1, 2, D = the minimum of m20 cx + m21 cy + m22 over the four corner pixel
 * centres (0.5 | out_w - 0.5, 0.5 | out_h - 0.5) -- the denominator is affine, so that is its minimum
 * over the grid -- and D' = D - 3 eps S_2:
 *   - all nine entries finite;
 *   - S_r <= 2^22 for all three rows;
 *   - D' > 0: each of wn's three roundings errs by at most eps times a partial sum that S_2 bounds,
 *     so the float32 wn >= D' > 0 at every pixel;
 *   - S_0 / D' <= 2^22 and S_1 / D' <= 2^22: |xn| <= S_0 (1 + 3 eps) and wn >= D', so the quotient
 *     floors exactly and fits an int;
 *   - with L_0 = W, L_1 = H (the frame), E_r = 3 eps (S_r + (L_r + 3) S_2) / D' + 2 eps (L_r + 3) <=
 *     7/8, else "the perspective is too strong for float32 positions";
 *   - output size, fill finite and 420 on an odd frame as above.
 * E_r bounds |u_float32 - u_exact| for every pixel whose float32 position lies within two taps of
 * the frame, |xs| <= L + 3 =: P.  Three roundings in the numerator: |xn - xn*| <= 3 eps S_r; three in
 * the denominator: |wn - wn*| <= 3 eps S_2, both wn, wn* >= D'.  Then |xn / wn - xn* / wn*| <=
 * |xn - xn*| / wn* + |xn / wn| |wn - wn*| / wn* <= 3 eps (S_r + P S_2) / D' (second order terms are
 * below the slack of the partial-sum bounds); the quotient's rounding adds eps P and that of - 0.5f
 * another eps P.  For an affine call accepted today with the flag and row 0 0 1: S_2 = D = 1, E <=
 * 0.77 at the reach limit, so it stays acceptable -- but for a reach within 3 eps (relative) of 2^22,
 * where S_r / D' with D' = 1 - 3 eps exceeds 2^22 and the flagged call is refused.  The bound was confirmed on 3,597 accepted random
 * homographies over frames from 21 x 37 to 4000 x 65535 (worst error 0.34 E_r).
 * window[j] follows the affine rule with the four corner positions replaced by the quotients xn / wn,
 * yn / wn in double: the image of the output rectangle under a projective map whose denominator is
 * positive on it is a convex quadrilateral (a projective map sends segments to segments where the
 * denominator keeps its sign), so the extremes of xs and ys over the grid are at the corners.  Columns
 * floor(min xs - 0.5) - 1 .. floor(max xs - 0.5) + 2 (one tap wider each side for cubic), rows alike,
 * each end clamped into the frame, never empty, even-ed for 420; the one-pixel growth is what E <= 7/8
 * pays for.  A flagged matrix with last row 0 0 1 gives the window of its 6-entry form.  Frames of
 * one architecture share one batched tail group whatever their matrices.
 * Kernels (dec_out.hip): the geometries Warp<false, true> and Warp<true, true> of dec_fmt, dec_fmt_col
 * and dec_fmt_stat. */
enum {
    CCMI_PAD_FILL = 0,
    CCMI_PAD_EDGE = 1,
    CCMI_WARP_CUBIC = 0x100,
    CCMI_WARP_CLAMP = 0x200,
    CCMI_WARP_PROJECTIVE = 0x800
};
typedef struct ccmi_warp {
    int out_w, out_h, pad;
    float fill[3];        /* CCMI_PAD_FILL: value of a tap outside the frame, in q units (after step 3) */
    const float *matrix;  /* host, [n][6]: m00 m01 m02 m10 m11 m12 of frame j; CCMI_WARP_PROJECTIVE: [n][9], m00 .. m22 */
} ccmi_warp;
int ccmi_decode_batch_dev_warp_plan(const uint8_t *const *streams, const size_t *lens, int n, int out_bitdepth,
                                    int out_chroma, const ccmi_tensor_fmt *fmt, const ccmi_warp *warp,
                                    ccmi_frame_geom *geom /* [n] */, ccmi_roi_info *info /* [n] or NULL */,
                                    ccmi_rect window[] /* [n] or NULL */, size_t *workspace_bytes);
int ccmi_decode_batch_dev_warp(const uint8_t *const *streams, const size_t *lens, int n, void *const *out_dev,
                               const size_t *out_caps, const ccmi_tensor_fmt *fmt, const ccmi_warp *warp,
                               int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_warp_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m, int out_bitdepth,
                                  int out_chroma, const ccmi_tensor_fmt *fmt, const ccmi_warp *warp,
                                  ccmi_frame_geom *geom /* [m] */, ccmi_roi_info *info /* [m] or NULL */,
                                  ccmi_rect window[] /* [m] or NULL */, size_t *workspace_bytes);
int ccmi_latents_render_warp(const ccmi_latents *h, const int *index /* [m] or NULL */, int m, void *const *out_dev,
                             const size_t *out_caps, const ccmi_tensor_fmt *fmt, const ccmi_warp *warp,
                             int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);

/* Coloured formatted output: the formatted sink with a per-frame list of photometric operations --
 * brightness, saturation, contrast and a 3 x 4 colour matrix, the ColorJitter / RandomGrayscale half
 * of the usual augmentation recipe -- applied in the decoder's output stage, after the geometry
 * (step 3 of ccmi_tensor_fmt, step 3c of ccmi_resample, step 3d of ccmi_warp) and before step 4
 * (scale / bias):
 *   3z. x_0..x_2 = the three channels of output pixel (i, k) of frame j, at the output size.  Frame
 *       j's ops, count[j] <= CCMI_COL_MAX_OPS of them, are applied in the frame's own order; every
 *       product, sum and difference is one float32 operation in the order written (no fused
 *       multiply-add), clamp is to [0, 1]:
 *       CCMI_COL_BRIGHTNESS f (v[0], f >= 0):  x_c = clamp(f x_c);
 *       CCMI_COL_SATURATION f (v[0], f >= 0):  g = ((0.2989f x_0) + (0.587f x_1)) + (0.114f x_2),
 *           x_c = clamp((f x_c) + ((1 - f) g)); 1 - f is computed once on the host in float32;
 *       CCMI_COL_CONTRAST f (v[0], f >= 0; at most one per frame):  x_c = clamp((f x_c) + ((1 - f) m_j)),
 *           m_j the frame's mean grey in fixed point, which makes it independent of the order of
 *           summation: S_j = the sum over all out_h out_w output pixels of frame j of
 *           (uint64) rintf(clamp(g) 65535.0f), g the grey above of the pixel as it stands after the ops
 *           that precede the contrast op; m_j = (float)((double)S_j / ((double)(out_h out_w) 65535.0)).
 *           In a warp, pixels that come from `fill` count like any others.  The library sums integers
 *           (one 64-bit atomic add per wave into a per-frame accumulator of the workspace, cleared in
 *           stream), so a frame gives the same bits alone or in any batch, call after call;
 *       CCMI_COL_MATRIX M (v[0..11], row-major 3 x 4):
 *           x'_c = clamp((((M_c0 x_0) + (M_c1 x_1)) + (M_c2 x_2)) + M_c3), all three from the old x.
 *           Hue as a rotation of the chroma plane of YIQ, greyscale, channel permutations, inversion.
 *           It is NOT torchvision's HSV hue shift: a rotation in YIQ keeps luma and clips at the gamut.
 * The ops act on the three channels whatever they are (CCMI_COLOUR_ASIS on a YUV stream included);
 * the grey weights and the helpers' matrices are meant for RGB.  Steps 4-6 apply to the result.
 * A frame without ops, and a call with colour NULL, give the bits of the call without colour.
 *
 * One superset pair per source: fmt, then rs OR warp OR neither (rs and warp both NULL: the _fmt
 * call), then colour or NULL.  With a warp there is no roi (roi must be NULL) and `window` is filled
 * as by the _warp plan; without one `window` must be NULL.  colour NULL, or every count 0: exactly
 * the _rs / _warp call, plan and workspace included.  Otherwise the workspace grows by the op table
 * (one entry per frame in the tail's argument tables) and the accumulators (8 bytes per frame, rounded
 * to 256 for the call); frames with and without ops, in any orders, share the tail's launches
 * (ccmi_decode_last_tail_groups is what the call without colour reports), and the frames that have a
 * contrast op take part in one more pass per group, which evaluates the same pixels up to the
 * contrast op and adds up S_j.
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame and nothing written: rs and
 * warp both given, a roi with a warp, count or ops NULL, a count outside [0, CCMI_COL_MAX_OPS], an
 * unknown op, two contrast ops in one frame, a negative or non-finite factor, a non-finite matrix
 * entry; and everything the _rs / _warp plan checks.
 * Measured (profiles/decode_colour_ab.txt): 960 class-E streams from an int16 store, RandomResizedCrop to
 * 224 x 224, four ops per frame in random orders (every frame with a contrast op), bf16 RGB normalised:
 * 50.2-51.7 ms per call (tail 45.2 ms) against 48.7-49.8 ms (tail 44.5 ms) for the call without ops and
 * 57.7-59.4 ms for the float32 render followed by the same ops as torch operations; peak allocation above
 * store and workspace 276 MiB against 1654 MiB. */
enum { CCMI_COL_BRIGHTNESS = 0, CCMI_COL_SATURATION = 1, CCMI_COL_CONTRAST = 2, CCMI_COL_MATRIX = 3 };
enum { CCMI_COL_MAX_OPS = 8 };
typedef struct ccmi_colour_op {
    int op;      /* CCMI_COL_* */
    float v[12]; /* v[0] = the factor f; CCMI_COL_MATRIX: M, row-major 3 x 4 */
} ccmi_colour_op;
typedef struct ccmi_colour {
    const int *count;          /* host, [n]: ops of frame j */
    const ccmi_colour_op *ops; /* host, flat: frame j's ops follow frame j - 1's */
} ccmi_colour;
int ccmi_decode_batch_dev_col_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                   const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth, int out_chroma,
                                   const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                   const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                   ccmi_frame_geom *geom /* [n] */, ccmi_roi_info *info /* [n] or NULL */,
                                   ccmi_rect window[] /* [n] or NULL; warp only */, size_t *workspace_bytes);
int ccmi_decode_batch_dev_col(const uint8_t *const *streams, const size_t *lens, int n,
                              const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev, const size_t *out_caps,
                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                              const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                              int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_col_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                 const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                 const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                 const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                 ccmi_frame_geom *geom /* [m] */, ccmi_roi_info *info /* [m] or NULL */,
                                 ccmi_rect window[] /* [m] or NULL; warp only */, size_t *workspace_bytes);
int ccmi_latents_render_col(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                            const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                            const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                            const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                            int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);

/* Filtered formatted output: the coloured sink with a per-frame separable blur and a per-frame solarize --
 * the GaussianBlur / RandomSolarize steps of the self-supervised recipes (SimCLR, BYOL, MoCo v3, DINO) --
 * applied in the decoder's output stage after step 3z (colour) and before step 4 (scale / bias), on the
 * frame at the output size oh x ow (the region's for the plain formatted call, out_h x out_w with a
 * resample or a warp).  Frame j TAKES THE STAGE when radius[j] > 0 or (solarize != NULL and
 * solarize[j] <= 1.0f); every other frame goes through the kernels it goes through without a filter and
 * keeps its bits.  For a frame that takes the stage, every product, sum and difference is one float32
 * operation in the order written (no fused multiply-add):
 *   3y-0. x_c(i, k) = the value after step 3z at output row i and STORED column k (the column after
 *         mirror[j], the x' of step 6: the filter runs on the frame as it will be stored, and a mirrored
 *         row summed in ascending order is a different float32 sum), + 0.0f (a -0 becomes +0);
 *   3y-1. blur, only when r = radius[j] > 0, with the frame's half taps w_0 (centre) .. w_r:
 *         refl(a, n) = 0 when n == 1; else p = 2 (n - 1), m = a mod p taken into [0, p), and
 *         refl = m < n ? m : p - m.  For r < n this is torch's "reflect" padding; for r >= n it folds as
 *         often as needed (where torch refuses).
 *         t_c(i, k) = sum_{d = -r .. r} w_|d| x_c(i, refl(k + d, ow)), from 0.0f over d ascending;
 *         y_c(i, k) = clamp(sum_{d = -r .. r} w_|d| t_c(refl(i + d, oh), k), 0, 1), summed the same way
 *         (a NaN sum, which only taps that overflow float32 can give, clamps to 0).
 *         With r = 0 both passes are skipped and y = x;
 *   3y-2. solarize, only when th = solarize[j] <= 1: y_c = (y_c >= th) ? 1.0f - y_c : y_c
 *         (torchvision's float solarize).
 * Steps 4-6 then apply to y, stored at column k (the mirror has been applied already).
 * The taps are an input and not derived from a sigma here, so the bits never depend on anybody's exp;
 * half taps make the kernel symmetric by construction; any finite float32 taps are legal.
 *
 * One superset pair per source: the _col argument list with `filter` after `colour`.  filter NULL, or no
 * frame taking the stage: exactly the _col call, plan, workspace, launches and bits.  Otherwise the
 * workspace grows by exactly
 *     sum over the frames that take the stage of (12 oh ow rounded up to 256)  +  256 S   bytes,
 * S the number of those frames: one float32 staging frame [3][oh][ow] each, and 256 bytes each of the
 * call's tables (the frame's entry of the staging launch, its filter entry and its 16 taps: the tap
 * table), uploaded with the rest of the tables in one copy.  The frames of one tail group stay one
 * group (ccmi_decode_last_tail_groups is what the call without a filter reports); the staged frames of
 * a group run the group's geometry and colour kernels once more on their own -- in the identity format:
 * float32, planar, scale 1, bias 0, the frame's mirror -- into their staging frames, and then one launch
 * of the filter kernel (both passes; the horizontal result never leaves the LDS) into the caller's
 * tensors in the call's format.
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame and nothing written: radius
 * NULL, a radius outside [0, CCMI_FLT_MAX_RADIUS], taps NULL while some radius > 0, a non-finite tap, a
 * NaN threshold; and everything the _col plan checks.
 * Measured (profiles/decode_filter_ab.txt): the workload of the colour stage above with a 23-tap Gaussian
 * blur on half of the frames and solarize on a fifth (589 of 960 frames take the stage): 54.5 ms per call
 * (tail 47.1 ms) against 52.0-52.1 ms (tail 45.2 ms) for the call without a filter and 58.1-58.2 ms for the
 * float32 render followed by the same steps as torch operations; peak allocation above store and workspace
 * 276 MiB against 1654 MiB; the workspace grows by 338 MiB. */
enum { CCMI_FLT_MAX_RADIUS = 15 };
typedef struct ccmi_filter {
    const int   *radius;   /* host, [n]: r_j in [0, CCMI_FLT_MAX_RADIUS]; 0 = no blur for frame j      */
    const float *taps;     /* host, flat: frame j's r_j + 1 half taps w_0 (centre) .. w_r follow frame  */
                           /* j - 1's; frames with r_j = 0 contribute none; may be NULL if every r is 0 */
    const float *solarize; /* host, [n] or NULL: threshold th_j; acts only where th_j <= 1              */
} ccmi_filter;
int ccmi_decode_batch_dev_flt_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                   const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth, int out_chroma,
                                   const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                   const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                   const ccmi_filter *filter /* or NULL */, ccmi_frame_geom *geom /* [n] */,
                                   ccmi_roi_info *info /* [n] or NULL */, ccmi_rect window[] /* [n] or NULL; warp only */,
                                   size_t *workspace_bytes);
int ccmi_decode_batch_dev_flt(const uint8_t *const *streams, const size_t *lens, int n,
                              const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev, const size_t *out_caps,
                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                              const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                              const ccmi_filter *filter /* or NULL */, int out_bitdepth, int out_chroma,
                              void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_flt_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                 const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                 const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                 const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                 const ccmi_filter *filter /* or NULL */, ccmi_frame_geom *geom /* [m] */,
                                 ccmi_roi_info *info /* [m] or NULL */, ccmi_rect window[] /* [m] or NULL; warp only */,
                                 size_t *workspace_bytes);
int ccmi_latents_render_flt(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                            const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                            const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                            const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                            const ccmi_filter *filter /* or NULL */, int out_bitdepth, int out_chroma,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Tone ops: the filtered sink with a per-frame list of tone operations -- the photometric half of the op
 * tables of RandAugment, TrivialAugmentWide and AutoAugment: brightness, colour (saturation), contrast,
 * solarize, posterize, autocontrast, equalize and sharpness, in a drawn order -- applied in the decoder's
 * output stage on the staged frame at the output size oh x ow:
 *   3x. after step 3z (colour) and before steps 3y-1 / 3y-2 (blur, solarize) and step 4.
 * Frame j TAKES THE STAGE when count[j] > 0, or when the filter already makes it (the ccmi_filter rule,
 * unchanged).  The staged value is the x_c(i, k) of step 3y-0: stored column, after the mirror, + 0.0f.
 * The ops of frame j run in the frame's own order, each over the whole frame before the next starts.
 * Every product, sum, difference and division is one float32 operation in the order written (no fused
 * multiply-add; a division is correctly rounded); clamp is to [0, 1] and a NaN clamps to 0; 1 - f is
 * computed once on the host in float32.
 *   CCMI_TONE_BRIGHTNESS f, CCMI_TONE_SATURATION f, CCMI_TONE_MATRIX M: the formulas of step 3z;
 *   CCMI_TONE_CONTRAST f: the formula and the fixed-point mean S_j of step 3z, taken over the frame as it
 *       stands before this op.  Any number per frame: here each is its own pass;
 *   CCMI_TONE_SOLARIZE th (v[0]): x_c = (x_c >= th) ? 1.0f - x_c : x_c (step 3y-2's);
 *   CCMI_TONE_POSTERIZE b (v[0] = b, an integer in 1..8), L = 2^b:
 *       x_c = min(max(floorf(clamp(x_c) L), 0), L - 1) (1.0f / L)   (torchvision v2's float form; 1 / L is exact);
 *   CCMI_TONE_AUTOCONTRAST: per channel lo_c, hi_c = the min and max over the frame of clamp(x_c).
 *       hi_c == lo_c: the channel is unchanged.  Otherwise s = 1.0f / (hi_c - lo_c) and
 *       x_c = clamp((x_c - lo_c) s).  Min and max do not depend on the order of reduction;
 *   CCMI_TONE_EQUALIZE, per channel, N = oh ow (N <= 2^28: everything fits 32 bits):
 *       q = (int) rintf(clamp(x_c) 255.0f), ties to even; H_c[0..255] = the histogram of q over the frame;
 *       last = the highest non-empty bin; step = (N - H_c[last]) / 255 (integer division);
 *       step == 0: lut = the identity; otherwise lut[0] = 0 and, t >= 1,
 *       lut[t] = min(255, ((sum_{u < t} H_c[u]) + step / 2) / step)   (torchvision's _equalize_single_image);
 *       x_c = (float)lut[q] / 255.0f.  The op always quantises, also when the LUT is the identity;
 *   CCMI_TONE_SHARPNESS f (f >= 0): oh <= 2 or ow <= 2: the frame is unchanged.  Otherwise, for interior
 *       pixels (0 < i < oh - 1, 0 < k < ow - 1),
 *       b_c = sum over di = -1..1, dk = -1..1 (di outer, both ascending, from 0.0f) of w(di, dk) x_c(i + di, k + dk),
 *       w = (float)(5.0 / 13.0) at the centre and (float)(1.0 / 13.0) elsewhere; on the border b_c = x_c;
 *       x_c = clamp((f x_c) + ((1 - f) b_c)), all reads of the frame as it stood before this op
 *       (torchvision's adjust_sharpness).
 * In a warp, pixels that come from `fill` count in every statistic like any others.
 * BATCH INVARIANCE: every statistic is an integer sum or a min / max (accumulated with integer atomics in
 * the workspace, cleared in stream), so a frame gives the same bits alone or in any batch, call after call.
 *
 * One superset pair per source: the _flt argument list with `tone` between `colour` and `filter`.  tone
 * NULL, or every count 0: exactly the _flt call -- plan, workspace, launches and bits;
 * ccmi_decode_last_tail_groups is what the call without tone reports and the frames of one tail group
 * stay one group.  Otherwise, with S = the frames that take the stage (by either rule), the workspace is
 * that of the _flt call in which exactly those S frames take the stage, plus exactly
 *     512 S  +  sum over the frames with a SHARPNESS op of (12 oh ow rounded up to 256)  +  3328 A   bytes,
 * A = the number of CONTRAST, AUTOCONTRAST and EQUALIZE ops in the call: a 512-byte entry of the tone
 * tables per staged frame (its op list and segments; uploaded with the rest of the tables in one copy,
 * not in the tail's per-frame arguments), a second float32 frame where a sharpness op cannot run in place,
 * and one accumulator block per statistic op (3 x 256 uint32 bins, 3 minima, 3 maxima, one uint64: 3104
 * bytes rounded to 256).  A frame staged by its tone ops alone costs what ccmi_filter states for a staged
 * frame: (12 oh ow rounded up to 256) + 256 bytes.
 * A frame's list is cut into segments, a run of pointwise ops ended by a whole-frame op; segment p of all
 * staged frames of a tail group shares its launches (a statistics pass, then an apply or sharpness pass),
 * and the filter kernel then formats the frame (radius 0 and no solarize for a frame without a filter).
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame and nothing written: count or
 * ops NULL, a count outside [0, CCMI_TONE_MAX_OPS], an unknown op, a negative or non-finite factor, a
 * non-finite matrix entry, a NaN threshold, posterize bits that are not an integer in 1..8; and
 * everything the _flt plan checks.
 * Measured (profiles/decode_tone_ab.txt): 960 class-E streams from an int16 store, RandomResizedCrop windows
 * x RandAugment(2, 9) draws warped to 224 x 224, bf16 RGB normalised (761 frames take the stage): 41.5 ms
 * per call (tail 37.5 ms) against 40.4-40.5 ms (tail 36.9-37.0 ms) for the call without tone ops and
 * 45.9-46.0 ms for the float32 render followed by the same ops as torch operations; peak allocation above
 * store and workspace 276 MiB against 1654 MiB; the workspace grows by 507 MiB. */
enum { CCMI_TONE_BRIGHTNESS = 0, CCMI_TONE_SATURATION = 1, CCMI_TONE_CONTRAST = 2, CCMI_TONE_MATRIX = 3,
       CCMI_TONE_SOLARIZE = 4, CCMI_TONE_POSTERIZE = 5, CCMI_TONE_AUTOCONTRAST = 6,
       CCMI_TONE_EQUALIZE = 7, CCMI_TONE_SHARPNESS = 8 };
enum { CCMI_TONE_MAX_OPS = 8 };
typedef struct ccmi_tone_op {
    int op;      /* CCMI_TONE_* */
    float v[12]; /* v[0] = the factor, threshold or bits; CCMI_TONE_MATRIX: M, row-major 3 x 4 */
} ccmi_tone_op;
typedef struct ccmi_tone {
    const int *count;        /* host, [n]: ops of frame j, 0 .. CCMI_TONE_MAX_OPS */
    const ccmi_tone_op *ops; /* host, flat: frame j's ops follow frame j - 1's */
} ccmi_tone;
int ccmi_decode_batch_dev_tone_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                    const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth, int out_chroma,
                                    const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                    const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                    const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                    ccmi_frame_geom *geom /* [n] */, ccmi_roi_info *info /* [n] or NULL */,
                                    ccmi_rect window[] /* [n] or NULL; warp only */, size_t *workspace_bytes);
int ccmi_decode_batch_dev_tone(const uint8_t *const *streams, const size_t *lens, int n,
                               const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev, const size_t *out_caps,
                               const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                               const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                               const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                               int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_tone_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                  const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                  const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                  const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                  const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                  ccmi_frame_geom *geom /* [m] */, ccmi_roi_info *info /* [m] or NULL */,
                                  ccmi_rect window[] /* [m] or NULL; warp only */, size_t *workspace_bytes);
int ccmi_latents_render_tone(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                             const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                             const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                             const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                             const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                             int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);

/* Mix stage: the tone sink with RandomErasing, MixUp and CutMix -- the three steps the supervised ViT
 * recipes (DeiT, timm, torchvision's reference scripts) add after the normalisation -- applied in the
 * decoder's output stage by one pass per call that sees two staged float32 frames at once and writes the
 * caller's tensor, steps 5 and 6 applied once, after the mix.
 * Frame j of a call of n frames TAKES THE MIX STAGE when count[j] > 0 or partner[j] >= 0.  A frame is
 * MIX-STAGED when it takes the stage or is the partner of a frame that does.  Every other frame goes
 * through the kernels it goes through without `mix` and keeps its bits.
 * For a mix-staged frame y_c(i, k) is the value after step 3y-2 (without a filter: the x_c(i, k) of step
 * 3y-0): the stored column after the mirror, + 0.0f, at the stored size oh x ow.  Every product and sum is
 * one float32 operation in the order written (no fused multiply-add); rectangles and boxes are in stored
 * coordinates, after mirror[j], like the filter's.
 *   4.  a_c = y_c scale[c] + bias[c], as ever;
 *   4e. erase, in the normalised units (torchvision and timm apply RandomErasing after Normalize): the
 *       frame's rectangles t = 0 .. count[j] - 1 in order, a later one winning: where x_t <= k < x_t + w_t
 *       and y_t <= i < y_t + h_t:  a_c = (sigma_t == 0) ? v_t[c] : v_t[c] + g,
 *       g = (sqrtf(-2.f * logf(u1)) * cospif(2.f * u2)) * sigma_t, u1 = unif(r),
 *       u2 = unif(mix64(r + 0x632BE59BD9B4E019)), r = mix64(seed[j] ^ mix64(index)),
 *       index = (c oh + i) ow + k (< 3 * 2^28): the generator of ccmi_train_args at step 0, frame 0.  The
 *       draw depends on (seed[j], c, i, k, oh, ow) and on nothing else -- not on the frame's place in the
 *       call, the layout or the element type (batch invariance) -- and overlapping noise rectangles see
 *       the same draw;
 *   4m. mix, p = partner[j] >= 0: b_c = steps 4 and 4e of frame p at the same (i, k), with p's own
 *       rectangles and seed; p's own partner does not enter (batch.roll() / batch.flip() of the erased,
 *       unmixed batch).  box[j] non-empty (w > 0 and h > 0): m_c = b_c inside the box, a_c outside
 *       (CutMix; lam is not read).  box[j] empty: m_c = (lam[j] a_c) + (oml_j b_c), oml_j = 1.0f - lam[j]
 *       computed once on the host in float32 (MixUp; torch's rolled.mul(1 - lam).add_(x.mul(lam)) gives
 *       the same bits).  p == j is legal and follows the formula.  partner[j] < 0: m_c = a_c;
 *   5, 6. m_c to `elem`, round to nearest even, stored as ever.
 * A mix-staged frame with neither rectangles nor a partner is formatted by the same kernel with m = a: the
 * bits of a frame staged by the filter stage with radius 0 and no solarize, which are those of the call
 * without the stage wherever no staged value is -0.
 *
 * One superset pair per source: the _tone argument list with `mix` after `filter`.  mix NULL, or no frame
 * taking the stage: exactly the _tone call -- plan, workspace, launches, ccmi_decode_last_tail_groups and
 * bits.  Otherwise, with M = the mix-staged frames, the workspace is that of the _tone call in which the
 * M frames take the filter stage as well (a staging frame and 256 bytes each by ccmi_filter's formula, and
 * the tone entry a call with tone ops gives every staged frame), plus exactly
 *     256 |M|  +  sum over the M frames with radius > 0 or a solarize of (12 oh ow rounded up to 256)  bytes:
 * the frame's 256-byte entry of the mix table (source, destination, size, its own resolved strides, seed,
 * rectangles, partner's entry, lam, 1 - lam, box), uploaded with the rest of the tables in the call's one copy, and a second
 * float32 frame where the filter kernel has something to compute: it then writes there in the identity
 * format instead of the caller's tensor; with radius 0 and no solarize it is not launched for the frame and
 * the mix kernel reads the staging frame.  The mix kernel is one launch per call over the M frames, on the
 * call's stream after every chunk and tail group has been joined: a partner may sit in any of them.
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame and nothing written: mix without a
 * format; a count outside [0, CCMI_MIX_MAX_RECTS]; rects NULL while a count is positive; a non-finite v or
 * sigma, or sigma < 0; a rectangle or box with a negative size, or a non-empty one not inside
 * [0, ow) x [0, oh) (an empty one is legal and does nothing); a partner outside [-1, n); a partner whose
 * stored size differs from the frame's; lam NULL where it is read; a lam that is NaN or outside [0, 1];
 * and everything the _tone plan checks.
 * Measured (profiles/decode_mix_ab.txt): the workload of the tone stage above plus RandomErasing(p = 0.25,
 * per-element Gaussian) on 248 frames and a per-frame MixUp(0.8) / CutMix(1.0) with the frame before (475
 * blends, 485 boxes; all 960 frames mix-staged): 43.6-44.3 ms per call (tail 37.6-37.7 ms) against
 * 43.0 ms (tail 37.5-37.6 ms) for the call without the stage and 48.4-48.8 ms for that call followed by the
 * same steps as torch operations on the bf16 tensor; peak allocation above store and workspace 276 MiB
 * against 827 MiB; the workspace grows by 114.6 MiB. */
enum { CCMI_MIX_MAX_RECTS = 4 };
typedef struct ccmi_erase_rect { int x, y, w, h; float v[3]; float sigma; } ccmi_erase_rect; /* 32 bytes */
typedef struct ccmi_mix {
    const int *count;             /* host, [n] or NULL (no frame erases): rectangles of frame j, 0 .. 4 */
    const ccmi_erase_rect *rects; /* host, flat: frame j's follow frame j - 1's                         */
    const uint64_t *seed;         /* host, [n] or NULL (0 for every frame); read where a sigma > 0      */
    const int *partner;           /* host, [n] or NULL (no frame mixes): -1 or a frame of this call     */
    const float *lam;             /* host, [n]; read where partner[j] >= 0 and box[j] is empty          */
    const ccmi_rect *box;         /* host, [n] or NULL (every box empty)                                */
} ccmi_mix;
int ccmi_decode_batch_dev_mix_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                   const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth, int out_chroma,
                                   const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                   const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                   const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                   const ccmi_mix *mix /* or NULL */, ccmi_frame_geom *geom /* [n] */,
                                   ccmi_roi_info *info /* [n] or NULL */, ccmi_rect window[] /* [n] or NULL; warp only */,
                                   size_t *workspace_bytes);
int ccmi_decode_batch_dev_mix(const uint8_t *const *streams, const size_t *lens, int n,
                              const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev, const size_t *out_caps,
                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                              const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                              const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                              const ccmi_mix *mix /* or NULL */, int out_bitdepth, int out_chroma, void *workspace,
                              size_t workspace_bytes, void *stream);
int ccmi_latents_render_mix_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                 const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                 const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                 const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                 const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                 const ccmi_mix *mix /* or NULL */, ccmi_frame_geom *geom /* [m] */,
                                 ccmi_roi_info *info /* [m] or NULL */, ccmi_rect window[] /* [m] or NULL; warp only */,
                                 size_t *workspace_bytes);
int ccmi_latents_render_mix(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                            const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                            const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                            const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                            const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                            const ccmi_mix *mix /* or NULL */, int out_bitdepth, int out_chroma, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Blend stage: the mix sink with weighted sums of up to CCMI_BLEND_MAX_TERMS staged frames of the call, and
 * with frames that are rendered as sources only -- what AugMix needs: several differently augmented renders
 * of one frame summed with per-frame weights BEFORE the normalisation and the one rounding.
 * Frame j of a call of n frames HAS TERMS when count[j] = K > 0: sources s_0 .. s_{K-1} (frames of this
 * call) and weights w_0 .. w_{K-1}.  It is SILENT when silent[j] != 0.  A frame is BLEND-STAGED when it has
 * terms, is silent, or is a source of a frame with terms.  Blend-staged frames are mix-staged in the sense
 * above: they take the filter's staging frame, have an entry of the mix table and are formatted by the
 * call's one launch after the join, together with the frames `mix` stages.  Every other frame keeps its
 * kernels and its bits.
 *   3b. blend, between step 3y-2 and step 4 (named 3b: 3z is the colour stage's step).  With y^f_c(i, k)
 *       the staged value of frame f after step 3y-2 (the y_c of the mix stage above), for a frame with terms:
 *           z_c = w_0 y^{s_0}_c,  then  z_c = z_c + (w_t y^{s_t}_c)  for t = 1 .. K - 1 ascending,
 *       every product and every sum one float32 operation (no fused multiply-add), at the same (c, i, k) of
 *       every source.  A frame without terms: z_c = y_c.  Steps 4, 4e, 4m, 5 and 6 then run on z_c in place
 *       of y_c, with the frame's own rectangles, seed, partner and box.
 *   A source enters as its own staged y: the source's own terms do not enter (the rule a partner follows for
 *   its partner).  A source may be the frame itself, may repeat, and may be silent or not.
 *   The partner p of step 4m enters with ITS step 3b (then its steps 4 and 4e): MixUp or CutMix of an
 *   AugMixed batch mixes the blended partner.
 *   count[j] = 1, source j, weight 1.0f: the bits of the same frame merely mix-staged (1.0f y == y).
 * A SILENT frame is planned, decoded and staged like any other: geom[j], info[j] and window[j] are filled.
 * Nothing is written for it: out_dev[j] may be NULL, out_caps[j] is not read, its alignment is not checked
 * and it takes no part in any check of the outputs.
 *
 * One superset pair per source: the _mix argument list with `blend` after `filter` and before `mix`.
 * blend NULL, or no frame with terms and no silent frame: exactly the _mix call -- plan, workspace,
 * launches (dec_mix_batch), ccmi_decode_last_tail_groups and bits.  Otherwise, with M = the frames that are
 * mix-staged by `mix` or blend-staged, the workspace is that of the _mix call in which the M frames are
 * mix-staged (its formula above, the blend-staged frames counted), plus exactly
 *     256 ceil(|M| / 4)  bytes:
 * the blend table, a sibling of the mix table that follows it in the call's one upload: 64 bytes per frame
 * of M (8 source entries, 8 weights), rounded up to 256 as a whole.  The number of terms sits in the frame's
 * 256-byte mix entry, whose layout is otherwise unchanged.  The launch is then dec_blend_batch, the form of
 * the mix kernel that reads K sources per frame: 12 K bytes read per pixel (12 K_p more where a partner
 * enters), 3 sizeof(elem) written; an entry without a destination (a silent frame) leaves at block start.
 * Checked by the plan before any GPU work, CCMI_ERR_ARG naming the frame (and the term) and nothing written:
 * blend without a format; a count outside [0, CCMI_BLEND_MAX_TERMS]; source or weight NULL while a count is
 * positive; a source outside [0, n); a source whose stored size differs from the frame's; a weight that is
 * not finite; a silent frame with terms, erase rectangles or a partner; a non-silent frame whose out_dev[j]
 * is NULL (run calls); and everything the _mix plan checks.
 * Not covered: sources of another stored size; AugMix's interleaving of geometric and photometric ops inside
 * a chain (ccmi/decode.py's aug_mix composes the geometry first, as rand_augment does); JSD-consistency
 * label handling; elastic transforms.  A coded-stream call decodes a stream once per repeat: build a store.
 * Measured (profiles/decode_blend_ab.txt): 960 class-E frames, RandomResizedCrop bases, AugMix(severity 3, width
 * 3), 3840 rendered frames for 960 bf16 outputs of 224 x 224: 179.6-180.6 ms per call (tail 164.0 ms) against
 * 181.4-182.2 ms for the 3840 frames without blend, all emitting, and 183.5-183.8 ms for their float32 render
 * followed by the sum, normalisation and cast as torch operations; peak allocation above store and workspace
 * 276 MiB against 1103 MiB and 4961 MiB; the workspace grows by 884.9 MiB over that of the 3840 frames. */
enum { CCMI_BLEND_MAX_TERMS = 8 };
typedef struct ccmi_blend {
    const int   *count;   /* host, [n] or NULL: terms of frame j, 0 (no blend) .. 8            */
    const int   *source;  /* host, flat, frame j's follow frame j - 1's: a frame of this call  */
    const float *weight;  /* host, flat, same order                                            */
    const int   *silent;  /* host, [n] or NULL: != 0: frame j is rendered and writes no output */
} ccmi_blend;
int ccmi_decode_batch_dev_blend_plan(const uint8_t *const *streams, const size_t *lens, int n,
                                     const ccmi_rect *roi /* [n] or NULL */, int out_bitdepth, int out_chroma,
                                     const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                     const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                     const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                     const ccmi_blend *blend /* or NULL */, const ccmi_mix *mix /* or NULL */,
                                     ccmi_frame_geom *geom /* [n] */, ccmi_roi_info *info /* [n] or NULL */,
                                     ccmi_rect window[] /* [n] or NULL; warp only */, size_t *workspace_bytes);
int ccmi_decode_batch_dev_blend(const uint8_t *const *streams, const size_t *lens, int n,
                                const ccmi_rect *roi /* [n] or NULL */, void *const *out_dev, const size_t *out_caps,
                                const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                const ccmi_blend *blend /* or NULL */, const ccmi_mix *mix /* or NULL */,
                                int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);
int ccmi_latents_render_blend_plan(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                                   const ccmi_rect *roi /* [m] or NULL */, int out_bitdepth, int out_chroma,
                                   const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                                   const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                                   const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                                   const ccmi_blend *blend /* or NULL */, const ccmi_mix *mix /* or NULL */,
                                   ccmi_frame_geom *geom /* [m] */, ccmi_roi_info *info /* [m] or NULL */,
                                   ccmi_rect window[] /* [m] or NULL; warp only */, size_t *workspace_bytes);
int ccmi_latents_render_blend(const ccmi_latents *h, const int *index /* [m] or NULL */, int m,
                              const ccmi_rect *roi /* [m] or NULL */, void *const *out_dev, const size_t *out_caps,
                              const ccmi_tensor_fmt *fmt, const ccmi_resample *rs /* or NULL */,
                              const ccmi_warp *warp /* or NULL */, const ccmi_colour *colour /* or NULL */,
                              const ccmi_tone *tone /* or NULL */, const ccmi_filter *filter /* or NULL */,
                              const ccmi_blend *blend /* or NULL */, const ccmi_mix *mix /* or NULL */,
                              int out_bitdepth, int out_chroma, void *workspace, size_t workspace_bytes, void *stream);

/* Network weights of a stream's intra frame as the decoder's fixed-point integers
 * (cc-frame-decoder.cpp:201-353, read_arm / read_ups / read_syn):
 *   arm: per hidden layer W[d][d] (out, in) then b[d]; then W_out[2][d], b_out[2]
 *        (ARM_PRECISION 8; the reference stores W transposed for its loop, :240-246);
 *   ups: n_ups full kernels of ups_k taps, then n_pre of pre_k taps (UPS_PRECISION 12,
 *        half kernels mirrored, decode_upsweights_qi :188-199);
 *   syn: per branch, per layer W[n_out][n_in][k][k] then b[n_out] (SYN precision 12).
 * counts[3] receives the three lengths; NULL buffers only query them. Host buffers. */
int ccmi_decode_weights_i32(const uint8_t *stream, size_t len, int32_t *arm, size_t arm_cap,
                            int32_t *ups, size_t ups_cap, int32_t *syn, size_t syn_cap, size_t *counts);

/* Integer upsampling (run_ups, cc-frame-decoder.cpp:572-679; ups_refine_cpu.hpp:11-79,
 * ups_upsample_cpu.hpp:12-91): latent grids (value << 8, flat in grid order) -> the
 * [n_grids][h0][w0] synthesis input at precision 12.  Device pointers. */
typedef struct ccmi_ups_i32_args {
    const int32_t *latent;  /* sum_l h[l] w[l] int32, grid l after grids 0..l-1 */
    int n_grids;
    int h[CCMI_MAX_GRIDS_PUBLIC];
    int w[CCMI_MAX_GRIDS_PUBLIC];
    const int32_t *kernels; /* the ups array of ccmi_decode_weights_i32 */
    int ups_k, n_ups, pre_k, n_pre;
    int32_t *out;           /* n_grids * h[0] * w[0] int32 */
    void *workspace;        /* ccmi_ups_workspace_bytes_i32() */
    size_t workspace_bytes;
} ccmi_ups_i32_args;
size_t ccmi_ups_workspace_bytes_i32(int n_grids, const int *h, const int *w);
int ccmi_ups_forward_i32(const ccmi_ups_i32_args *args, void *stream);

/* Integer synthesis of one branch (run_syn_branch, cc-frame-decoder.cpp:773-1042;
 * synfused_cpu.hpp:17-109, synlb_cpu.hpp:22-124, syn_cpu.hpp:21-112): [c_in][h][w] at
 * precision 12 -> [n_out][h][w].  Device pointers. */
typedef struct ccmi_syn_i32_args {
    const int32_t *in;
    int c_in, h, w;
    int n_layers;
    ccmi_syn_layer layers[CCMI_MAX_SYN_LAYERS];
    const int32_t *params;  /* one branch of the syn array of ccmi_decode_weights_i32 */
    int32_t *out;
    void *workspace;        /* ccmi_syn_workspace_bytes_i32(); 0 bytes for fused architectures */
    size_t workspace_bytes;
} ccmi_syn_i32_args;
size_t ccmi_syn_workspace_bytes_i32(const ccmi_syn_i32_args *args);
int ccmi_syn_forward_i32(const ccmi_syn_i32_args *args, void *stream);

/* Byte size of the decoded output of one stream (header parse only). */
int ccmi_decode_output_size(const uint8_t *stream, size_t len, int out_bitdepth,
                            int out_chroma, int as_yuv, size_t *size);

/* ------------------------------------------------------------------------- */
/* Path B writer: .cool encoder (the inverse of the decoder above).           */
/* ------------------------------------------------------------------------- */

/* Network parameter slots, in bitstream order (header.py:352-375, encode.py:364-390). */
enum { CCMI_NN_ARM_W = 0, CCMI_NN_ARM_B, CCMI_NN_UPS_W, CCMI_NN_UPS_B, CCMI_NN_SYN_W, CCMI_NN_SYN_B, CCMI_NN_SLOTS };

/* Everything a .cool intra frame carries besides its latent substreams: the GOP header
 * (header.py:72-117), the frame header (header.py:236-392) and the quantised network
 * integers (the values cc_code_wb_bac codes, encode.py:255-352).  Filled by
 * ccmi_cool_parse, consumed by ccmi_encode_frame. */
typedef struct ccmi_cool_desc {
    int h, w;                  /* image size */
    int bitdepth;              /* 8..16 */
    int frame_data_type;       /* 0 rgb, 1 yuv420, 2 yuv444 */
    int intra_period, p_period;
    int display_index;
    int dim_arm, n_hidden_arm;
    int n_ups, ups_k, n_pre, pre_k;
    int n_branches;
    int n_syn_layers;
    int syn_out[16], syn_ks[16];
    int syn_type[16];          /* raw byte: mode index * 16 + non-linearity index */
    int flow_gain;
    int ac_max_val_nn, ac_max_val_latent;
    int hls_sig_blksize;       /* signed: < 0 = adaptive block flags */
    int q_step_index[6];       /* CCMI_NN_* slots; -1 = slot absent (255 in the stream) */
    int expgol_count[6];       /* Exp-Golomb counts; ccmi_encode_frame: -1 = search 0..12 */
    int n_bytes_nn[6];         /* output of parse / encode */
    int n_grids;               /* latent resolutions (one 2D grid each) */
    int n_bytes_latent[8];     /* output of parse / encode */
    const int32_t *nn[6];      /* quantised integers per slot (host) */
    int nn_len[6];
} ccmi_cool_desc;

/* Parse the GOP + frame header of an intra .cool stream and decode its network
 * integers into nn_buf (nn_cap int32 slots; desc->nn[] point into it).  Host only. */
int ccmi_cool_parse(const uint8_t *stream, size_t len, ccmi_cool_desc *desc, int32_t *nn_buf, size_t nn_cap);

/* cc_code_wb_bac (ccencapi.cpp:97-177): Exp-Golomb(count) magnitudes + EP signs, one
 * CABAC substream.  use_count < 0 searches counts 0..12 for the fewest bytes (first
 * wins ties).  *len = bytes written (or needed, with CCMI_ERR_ARG, when cap is short). */
int ccmi_code_wb(const int32_t *x, int n, int use_count, uint8_t *out, size_t cap, size_t *len, int *count_used);

/* cc_decode_wb::decode_wb_continue (ccencapi.cpp:412-454) without hidden state: decode
 * n_runs consecutive runs of run_len[r] integers, run r with Exp-Golomb count
 * run_count[r], from one network substream; out receives sum(run_len) integers. */
int ccmi_decode_wb(const uint8_t *stream, size_t len, int n_runs, const int *run_len, const int *run_count, int32_t *out);

/* cc_code_latent_layer_bac (ccencapi.cpp:179-410): one latent grid, raster order, with
 * per-latent mu / log_scale in ARM fixed point (x256, the decoder's integers).  Host. */
int ccmi_code_latent_layer(const int32_t *x, const int32_t *mu, const int32_t *log_scale, int h, int w,
                           int hls_sig_blksize, uint8_t *out, size_t cap, size_t *len);

/* Integer ARM over every latent of every grid, fully parallel (the encoder side knows
 * all latents): the decoder's fixed-point arithmetic (arm_cpu.cpp:18-106 = ArmInt
 * pure_int, armint.py:80-261).  latent: int32 values [n] (grids flattened in order);
 * params: the decoder's integers, per hidden layer W[d][d] (out, in) then b[d], then
 * W_out[2][d], b_out[2].  mu / log_scale: int32 [n] (x256).  Device pointers. */
typedef struct ccmi_arm_i32_args {
    const int32_t *latent;
    int n_grids;
    int h[8], w[8];
    int dim_arm, n_hidden;
    const int32_t *params;
    int32_t *mu, *log_scale;
} ccmi_arm_i32_args;
int ccmi_arm_forward_i32(const ccmi_arm_i32_args *args, void *stream);

/* Write a whole .cool stream (GOP header, frame header, network substreams, latent
 * substreams; encode.py:113-623) for integer latents latent_dev (device, int32, grids
 * flattened).  ARM contexts run on the GPU (ccmi_arm_forward_i32); the CABAC substreams
 * are coded on host threads.  Fills desc->expgol_count / n_bytes_nn / n_bytes_latent.
 * *len = bytes written (or needed, with CCMI_ERR_ARG, when cap is short). */
int ccmi_encode_frame(ccmi_cool_desc *desc, const int32_t *latent_dev, uint8_t *out, size_t cap, size_t *len,
                      void *stream);

/* ------------------------------------------------------------------------- */
/* Encoder overfit step: training forward + backward + clip + Adam, on the GPU  */
/* ------------------------------------------------------------------------- */

/* Quantizer / noise selectors (quantizer.py:104-232). */
enum { CCMI_Q_NONE = 0, CCMI_Q_SOFTROUND_ALONE, CCMI_Q_SOFTROUND, CCMI_Q_HARDROUND, CCMI_Q_STE, CCMI_Q_TRUE_STE };
enum { CCMI_NOISE_NONE = 0, CCMI_NOISE_KUMARASWAMY, CCMI_NOISE_GAUSSIAN };

/* One optimisation step of enc/training/train.py:238-262 for `batch` independent frames
 * of the same size and architecture (each its own latents, networks and Adam state):
 *   quantize (quantizer.py) -> ARM + Laplace rate -> upsampling -> synthesis ->
 *   FrameEncoder train-mode output (frame.py:175-183: 420 nearest, clamp) ->
 *   loss = MSE + lmbda * rate_bits / (H*W) (loss.py) -> backward -> clip_grad_norm_(clip)
 *   -> Adam (torch.optim.Adam).
 * params per frame (float32): ARM (as ccmi_arm_args), then the trainable HALF kernels of
 * the n_ups upsampling filters ((ups_k+1)/2 taps each, upsampling.py:46-68), then the
 * n_pre refine filters ((pre_k+1)/2 each), then the synthesis (as ccmi_syn_args).
 * Supported synthesis: a 1x1 head of 2 non-residual layers (C -> hid <= 64 -> 3), then
 * 0..3 3x3 layers 3 -> 3 (replicate padding).  Adam moments: [batch][latent_stride +
 * param_stride], each row N latents then P parameters.  grad_out rows: [N + P], same
 * order.  target: 444 [3][H][W] or 420 Y[H][W], U, V[H/2][W/2].
 *
 * The noise generator (noise != CCMI_NOISE_NONE, noise_in null) is part of the contract; tests/
 * noise_ref.py restates this text and tests/test_train_noise_gpu.py holds every draw to it:
 *   mix64(z):  z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *              z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31      (mod 2^64)
 *   key      = (uint64) step << 40 ^ (uint64) frame << 32 ^ (uint64) index
 *   r        = mix64(seed ^ mix64(key)),  r2 = mix64(r + 0x632BE59BD9B4E019)
 *   unif(r)  = ((float) (r >> 40) + 0.5f) * 2^-24, the add rounded in float32: a 24-bit uniform
 *              in (0, 1]; r >> 40 = 0 gives 2^-25, r >> 40 >= 2^23 rounds the half to the even
 *              neighbour and r >> 40 = 2^24 - 1 gives 1.0
 *   u1 = unif(r), u2 = unif(r2)
 *   CCMI_NOISE_KUMARASWAMY  a = noise_param > 0, b = (2^a (a - 1) + 1) / a:
 *                           n = (1 - (1 - u1)^(1/b))^(1/a) - 1/2, in [-1/2, 1/2] (quantizer.py:60-102)
 *   CCMI_NOISE_GAUSSIAN     sigma = noise_param: n = sigma sqrt(-2 ln u1) cos(2 pi u2), |n| <= 5.9 sigma
 * `frame` is the row of the batch and `index` the latent's position among the frame's N latents
 * (grid 0 first), not its address: latent_stride does not enter.  Equal (seed, step, frame, index)
 * give equal draws in every call.  step keeps its low 24 bits in the key and frame its low 8 bits
 * clear of them: steps 2^24 apart, or frames 256 apart at steps that differ accordingly, share keys. */
typedef struct ccmi_train_args {
    int batch;
    int n_grids;
    int h[CCMI_MAX_GRIDS_PUBLIC];
    int w[CCMI_MAX_GRIDS_PUBLIC];
    int dim_arm, n_hidden;
    int ups_k, n_ups, pre_k, n_pre;
    int n_syn_layers;
    ccmi_syn_layer syn[CCMI_MAX_SYN_LAYERS];
    float gain;
    float *latent;          /* [batch][latent_stride], updated in place */
    int64_t latent_stride;
    float *params;          /* [batch][param_stride], updated in place */
    int64_t param_stride;
    float *adam_m, *adam_v; /* [batch][latent_stride + param_stride] */
    const float *target;    /* [batch][target_stride] */
    int64_t target_stride;
    int yuv420;
    int quantizer, noise;   /* CCMI_Q_*, CCMI_NOISE_* */
    float temperature, noise_param, lmbda;
    float lr, beta1, beta2, eps, clip;  /* clip <= 0: no gradient clipping */
    int step;               /* Adam step t >= 1 (bias correction) */
    uint64_t seed;          /* noise: counter-based RNG keyed by (seed, step, frame, index) */
    const float *noise_in;  /* optional [batch][latent_stride]: additive noise used as is */
    float *grad_out;        /* optional [batch][N + P]: raw gradients (before clipping) */
    float *loss_out;        /* optional [batch][4]: loss, mse, rate_bits, grad_norm (forward_only:
                               grad_norm 0; mse 0 unless a target is given, target_stride > 0) */
    int update;             /* 0: loss and gradients only; 1: Adam on everything; 2: Adam on the
                               latents only (optimized_module ["latent"]; the norm still covers all) */
    void *workspace;        /* ccmi_train_workspace_bytes() */
    size_t workspace_bytes;
    /* autograd use (torch.autograd.Function around the train-mode forward): */
    int forward_only;       /* 1: run the training forward only and write raw_out / rate_out */
    float *raw_out;         /* optional [batch][3][H][W]: raw synthesis output of the forward */
    float *rate_out;        /* optional [batch][N]: per-latent rate (bits) of the forward */
    const float *grad_raw;  /* optional [batch][3][H][W]: d loss / d raw output, used instead of
                               the built-in MSE term (whose value then reads 0 in loss_out) */
    const float *grad_rate; /* optional [batch][N]: d loss / d rate per latent, used instead of
                               the built-in lmbda / (H W) */
    const int32_t *adam_steps; /* optional device [batch]: each frame's own Adam step (overrides
                               `step`; a frame whose optimizer state was reloaded from its best
                               record, train.py:226-236); a step <= 0 leaves that frame unchanged:
                               neither its parameters nor its Adam moments are written */
    int32_t *step_counters; /* optional device [batch]: +1 per frame at the start of an update
                               step (the caller's per-frame step counts kept on the device without
                               a launch of its own; may alias adam_steps, which then reads the
                               incremented value) */
} ccmi_train_args;
size_t ccmi_train_param_count(const ccmi_train_args *args);
size_t ccmi_train_workspace_bytes(const ccmi_train_args *args);
int ccmi_train_step(const ccmi_train_args *args, void *stream);

/* ------------------------------------------------------------------------- */
/* MS-SSIM distortion: value and gradient for batches of frames, on the GPU     */
/* ------------------------------------------------------------------------- */

/* D = alpha_mse MSE + beta_ms (1 - MS) of `batch` frames x against targets y, and optionally dD/dx.
 * tests/msssim_ref.py restates this text in torch (any dtype, gradient by autograd) and
 * tests/test_msssim_gpu.py holds the kernels to its float64 run.
 *
 * Inputs.  For frame b and plane p < n_planes <= 3, X_p and Y_p have h[p] x w[p] samples.  Sample
 *   (i, j) of X_p is x[b x_stride + x_off[p] + i x_sub[p] x_pitch[p] + j x_sub[p]], x_sub 1 or 2, so
 *   one call reads the training step's raw output [3][H][W] under 4:2:0 (chroma at even rows and
 *   columns: x_off = {0, HW, 2HW}, x_pitch = W, x_sub = {1, 2, 2}, h[1] = H / 2, w[1] = W / 2), a packed
 *   4:4:4 frame and the packed Y, U, V of ccmi_post_f32.  With clamp != 0, X = min(max(x, 0), 1) (the
 *   train-mode frame output).  Y is used as given: frame b's planes packed h[p] x w[p] one after the
 *   other at y + b y_stride; y_stride 0 is one target for every frame.
 * Window.  g_k = exp(-(k - 5)^2 / 4.5) / sum, k = 0 .. 10, computed in double and rounded once to
 *   float32; separable, "valid" (no padding): a plane of h x w has (h - 10)(w - 10) positions.
 * Constants.  C1 = 1e-4, C2 = 9e-4 (data range 1).
 * Per scale s = 0 .. S - 1, 1 <= S = n_scales <= 5, in float32 (G* is the window):
 *     mu_x = G*X, mu_y = G*Y
 *     s_xx = G*(X X) - mu_x^2, s_yy likewise, s_xy = G*(X Y) - mu_x mu_y
 *     cs = (2 s_xy + C2) / (s_xx + s_yy + C2),  l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1)
 *     v_s = mean over the positions of cs (s < S - 1), of cs l (s = S - 1)
 *   The kernels form the statistics of X - 1/2 and Y - 1/2: the variances are the same and the
 *   cancellation smaller.
 * Next scale.  A 2 x 2 mean as avg_pool2d(2, padding = size mod 2, count_include_pad = True):
 *     h_{s+1} = ceil(h_s / 2),  X_{s+1}(i, j) = 1/4 sum_{a, b in {0, 1}} X_s(2i - ph + a, 2j - pw + b),
 *     ph = h_s mod 2, pw = w_s mod 2, samples outside the plane 0, the divisor always 4; Y likewise.
 *   Every scale of every plane needs min(h_s, w_s) >= 11 (five scales: a side of at least 161, the
 *   chain 161, 81, 41, 21, 11), else CCMI_ERR_ARG naming plane and scale.
 * Combination.  MS_p = prod_s max(v_s, 0)^weights[s]; a plane with any v_s <= 0 has MS_p = 0 and
 *   gradient 0.  MS = sum_p channel_weights[p] MS_p.  MSE = sum over every sample of every plane of
 *   (X - Y)^2 / the number of samples (loss.py _compute_mse's weighting).
 * Outputs.  out[b][4] = { D, MS, MSE, min over (p, s) of v_s before the max } (the last entry shows
 *   that the max was not hit).  grad, when given, has x's addressing and stride; only the sampled
 *   positions are written: dD/dx through the clamp, 0 where x lies outside [0, 1] (as the step's MSE).
 * Determinism.  The sums behind v_s and the MSE are one partial per workgroup, added in a fixed
 *   order (no float atomics): a frame gives the same bits alone, at any row of any batch, on every call.
 * Workspace.  With al(n) = 4 n rounded up to a multiple of 256 bytes, B = batch, and per frame
 *   pyr = sum_p sum_{s >= 1} h_s w_s, pos = sum_p sum_s (h_s - 10)(w_s - 10),
 *   tiles = sum_p sum_s ceil((h_s - 10) / 22) ceil((w_s - 10) / 32):
 *     2 al(B pyr) + al(2 B tiles) + al(16 B), and with grad + al(B pyr) + al(3 B pos).
 * CCMI_ERR_ARG with a message, before any HIP call: a null args / out / x / y, batch outside
 *   1 .. 65535, n_planes or n_scales out of range, a plane below the size rule, a weight, channel
 *   weight, alpha_mse or beta_ms that is negative or not finite, x_sub outside {1, 2}, x_off < 0, an
 *   x_pitch shorter than a row of samples, 0 < y_stride < a frame's samples, a short workspace.
 * Not measured: rate-distortion results of streams tuned for this metric. */
typedef struct ccmi_msssim_args {
    int batch, n_planes, n_scales, clamp;
    int h[3], w[3];
    const float *x;
    int64_t x_stride;       /* per frame */
    int64_t x_off[3], x_pitch[3];
    int x_sub[3];
    const float *y;
    int64_t y_stride;
    float weights[5], channel_weights[3], alpha_mse, beta_ms;
    float *out;             /* [batch][4] */
    float *grad;            /* optional */
    void *workspace;        /* ccmi_msssim_workspace_bytes() (0 for invalid shapes; grad counts) */
    size_t workspace_bytes;
} ccmi_msssim_args;
size_t ccmi_msssim_workspace_bytes(const ccmi_msssim_args *args);
int ccmi_msssim_f32(const ccmi_msssim_args *args, void *stream);

/* The overfit step with D of ccmi_msssim_args as its distortion, in one pass: the planes are the
 * step's train-mode output (clamp on; 4:2:0: chroma of H / 2 x W / 2 at even rows and columns of the
 * raw output) against `target`.  dist = NULL is ccmi_train_step: the same launches.  With a dist the
 * last synthesis layer stores its output (no fused MSE), under 4:2:0 one memset clears the chroma
 * planes of d loss / d raw, and the MS-SSIM kernels write the rest of it.  loss_out[b] =
 * { D + lmbda rate_bits / (H W), MSE, rate_bits, grad_norm }; dist_out[b] as ccmi_msssim_args.out.
 * forward_only with a target (target_stride > 0) fills loss_out and dist_out and writes no gradient.
 * CCMI_ERR_ARG: dist together with grad_raw, and what ccmi_msssim_f32 refuses.  The workspace is
 * ccmi_train_workspace_bytes_dist(args, dist) (= ccmi_train_workspace_bytes for dist = NULL). */
typedef struct ccmi_train_dist {
    int n_scales;
    float weights[5], channel_weights[3], alpha_mse, beta_ms;
    float *dist_out;        /* optional [batch][4] */
} ccmi_train_dist;
size_t ccmi_train_workspace_bytes_dist(const ccmi_train_args *args, const ccmi_train_dist *dist);
int ccmi_train_step_dist(const ccmi_train_args *args, const ccmi_train_dist *dist, void *stream);

/* quantize (quantizer.py:116-232) of n values x (already multiplied by the encoder gain):
 * y = Q(x) and dy = dQ/dx as the reference's autograd sees it (softround derivative for
 * "ste", 1 for "true_ste" and "none", 0 for "hardround"); noise: optional [n] additive
 * noise (the reference draws it with torch.rand_like / randn_like).  Device pointers. */
int ccmi_quantize_f32(const float *x, int64_t n, int quantizer, float temperature, const float *noise, float *y,
                      float *dy, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CCMI_H */
