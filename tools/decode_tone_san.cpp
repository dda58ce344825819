// decode_tone_san.cpp -- stand-alone host program for a sanitizer run of the tone stage's planning
// (ccmi_tone; decode_plan, dec_plan.cpp) on a machine without a GPU, in the form of
// decode_filter_san.cpp.  The plan walks the caller's flat op array by per-frame counts, so the counts
// and the ops sit in heap blocks of exactly their sizes (no block at all when every count is 0): a
// read past an end is reported.  Over the streams named on the command line, as streams and as a
// plan-only latent handle, on every geometry (whole frame, regions, a resample, a warp), with and
// without colour ops and a filter: valid lists (no ops, pointwise ops only, statistics, sharpness,
// the longest list, mixed batches), every rejected one (count or ops NULL, a count out of range, an
// unknown op, a negative or non-finite factor, a non-finite matrix entry, a NaN threshold, bad
// posterize bits), and the run entry points with lists the plan rejects or a plan-only handle
// (refused before any GPU work).  The workspace growth is checked against the formula of ccmi.h.
// No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_tone_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_tone.hip \
//       csrc/dec_latents.hip -o /tmp/decode_tone_san
//   /tmp/decode_tone_san $(find ../tests/golden/cool -name '*.cool')
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../cool-chic_amd/csrc/ccmi_internal.h"

// the float forward path is not linked: ccmi_api.cpp only needs the symbols
int ccmi_launch_arm_f32(const ccmi_arm_args *, hipStream_t, int) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_ups_f32(const ccmi_ups_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_syn_f32(const ccmi_syn_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_post_f32(const ccmi_post_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }

namespace {

long g_calls = 0, g_ok = 0, g_refused = 0;

void fail(const char *what)
{
    fprintf(stderr, "decode_tone_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

ccmi_tone_op op(int code, float v0 = 0.f)
{
    ccmi_tone_op o{};
    o.op = code, o.v[0] = v0;
    return o;
}

// a ccmi_tone whose arrays are heap blocks of exactly their sizes
struct Tone {
    ccmi_tone t{};
    int *count = nullptr;
    ccmi_tone_op *ops = nullptr;
    std::vector<size_t> first; // frame j's first op in the flat array
    explicit Tone(const std::vector<std::vector<ccmi_tone_op>> &lists)
    {
        const int n = (int)lists.size();
        count = static_cast<int *>(malloc(sizeof(int) * n));
        size_t total = 0;
        for (int i = 0; i < n; ++i) {
            first.push_back(total);
            count[i] = (int)lists[i].size();
            total += lists[i].size();
        }
        if (total) ops = static_cast<ccmi_tone_op *>(malloc(sizeof(ccmi_tone_op) * total));
        for (int i = 0; i < n; ++i)
            for (size_t k = 0; k < lists[i].size(); ++k) ops[first[i] + k] = lists[i][k];
        t.count = count, t.ops = ops;
    }
    ~Tone()
    {
        free(count);
        free(ops);
    }
    Tone(const Tone &) = delete;
};

struct Batch {
    std::vector<const uint8_t *> sp;
    std::vector<size_t> ln;
    ccmi_latents *h = nullptr;
    int n() const { return (int)sp.size(); }
};

struct Geo {
    const ccmi_rect *roi;
    const ccmi_resample *rs;
    const ccmi_warp *warp;
};

// both sources' plans of one tone on one geometry; returns the streams' rc, *need its workspace
int plan(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_colour *col, const ccmi_tone *tone,
         const ccmi_filter *flt, std::vector<ccmi_frame_geom> &geom, size_t *need)
{
    const int n = b.n();
    std::vector<ccmi_roi_info> info(n);
    std::vector<ccmi_rect> win(n);
    *need = 0;
    const int rc = ccmi_decode_batch_dev_tone_plan(b.sp.data(), b.ln.data(), n, g.roi, 0, 444, &fmt, g.rs, g.warp, col, tone,
                                                   flt, geom.data(), info.data(), g.warp ? win.data() : nullptr, need);
    ++g_calls;
    size_t need_h = 0;
    std::vector<ccmi_frame_geom> geom_h(n);
    const int rc_h = ccmi_latents_render_tone_plan(b.h, nullptr, n, g.roi, 0, 444, &fmt, g.rs, g.warp, col, tone, flt,
                                                   geom_h.data(), nullptr, nullptr, &need_h);
    ++g_calls;
    if (rc != rc_h) fail("the two sources disagree on a tone list");
    if (rc == CCMI_OK) g_ok += 2;
    return rc;
}

// a tone the plan must refuse, naming `frame`: both plans, then both run entry points, which must
// refuse as well before they touch the made-up output pointers
void refused(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_tone &tone, int frame)
{
    const int n = b.n();
    std::vector<ccmi_frame_geom> geom(n);
    size_t need = 0;
    if (plan(b, g, fmt, nullptr, &tone, nullptr, geom, &need) != CCMI_ERR_ARG) fail("a bad tone list was not refused");
    char want[32];
    snprintf(want, sizeof want, "frame %d", frame);
    if (!strstr(ccmi_last_error(), want)) fail("the refusal does not name the frame");
    if (need != 0) fail("a refused plan wrote a workspace size");
    std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
    std::vector<size_t> caps(n, size_t(1) << 30);
    if (ccmi_decode_batch_dev_tone(b.sp.data(), b.ln.data(), n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr,
                                   &tone, nullptr, 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
        fail("the run entry point took a bad tone list");
    if (ccmi_latents_render_tone(b.h, nullptr, n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr, &tone, nullptr,
                                 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
        fail("the render entry point ran on a plan-only handle");
    g_calls += 2;
    ++g_refused;
}

size_t r256(size_t v) { return (v + 255) / 256 * 256; }

void run_batch(const Batch &b)
{
    const int n = b.n();
    ccmi_tensor_fmt fmt{};
    fmt.elem = CCMI_ELEM_BF16, fmt.colour = CCMI_COLOUR_RGB;
    for (int c = 0; c < 3; ++c) fmt.scale[c] = 4.f + c, fmt.bias[c] = -1.f;
    uint8_t *mir = static_cast<uint8_t *>(malloc(n));
    for (int i = 0; i < n; ++i) mir[i] = (uint8_t)(i & 1);
    fmt.mirror = mir;
    std::vector<ccmi_rect> rects(n);
    for (int i = 0; i < n; ++i) rects[i] = ccmi_rect{2 * (i % 3), 4, 33 + 2 * (i % 5), 17 + (i % 4)};
    const ccmi_resample rs{29, 13, CCMI_FILTER_TRIANGLE};
    float *mat = static_cast<float *>(malloc(sizeof(float) * 6 * n));
    for (int i = 0; i < n; ++i) {
        const float m[6] = {0.5f, 0.1f * (float)(i % 3), 3.f, -0.1f, 0.5f, 2.f};
        memcpy(mat + 6 * i, m, sizeof m);
    }
    ccmi_warp wp{};
    wp.out_w = 29, wp.out_h = 13, wp.pad = CCMI_PAD_EDGE, wp.matrix = mat;
    // colour ops: one brightness op per frame, every third frame a contrast op as well
    int *counts = static_cast<int *>(malloc(sizeof(int) * n));
    int n_ops = 0;
    for (int i = 0; i < n; ++i) n_ops += counts[i] = 1 + (i % 3 == 0);
    ccmi_colour_op *cops = static_cast<ccmi_colour_op *>(calloc(n_ops, sizeof(ccmi_colour_op)));
    for (int i = 0, k = 0; i < n; ++i) {
        cops[k].op = CCMI_COL_BRIGHTNESS, cops[k++].v[0] = 1.1f;
        if (i % 3 == 0) cops[k].op = CCMI_COL_CONTRAST, cops[k++].v[0] = 0.7f;
    }
    const ccmi_colour col{counts, cops};
    // a filter that stages every fourth frame (a blur) and every fourth + 1 (solarize)
    int *radius = static_cast<int *>(malloc(sizeof(int) * n));
    float *th = static_cast<float *>(malloc(sizeof(float) * n));
    int n_blur = 0;
    for (int i = 0; i < n; ++i) n_blur += (radius[i] = i % 4 == 0 ? 2 : 0) > 0, th[i] = i % 4 == 1 ? 0.5f : 2.f;
    float *taps = static_cast<float *>(malloc(sizeof(float) * 3 * (n_blur ? n_blur : 1)));
    for (int k = 0; k < 3 * n_blur; ++k) taps[k] = 0.2f;
    const ccmi_filter flt{radius, taps, th};

    // the kinds of list a frame can have
    ccmi_tone_op mx = op(CCMI_TONE_MATRIX);
    for (int e = 0; e < 12; ++e) mx.v[e] = e % 5 == 0 ? 1.f : 0.f;
    const std::vector<ccmi_tone_op> none, point = {op(CCMI_TONE_BRIGHTNESS, 1.1f), op(CCMI_TONE_POSTERIZE, 4.f), mx,
                                                   op(CCMI_TONE_SOLARIZE, 0.5f), op(CCMI_TONE_SATURATION, 0.f)},
                                    stats = {op(CCMI_TONE_EQUALIZE), op(CCMI_TONE_BRIGHTNESS, 0.9f), op(CCMI_TONE_CONTRAST, 1.2f),
                                             op(CCMI_TONE_AUTOCONTRAST), op(CCMI_TONE_EQUALIZE)},
                                    sharp = {op(CCMI_TONE_SHARPNESS, 1.5f), op(CCMI_TONE_CONTRAST, 0.7f),
                                             op(CCMI_TONE_SHARPNESS, 0.f)},
                                    longest(CCMI_TONE_MAX_OPS, op(CCMI_TONE_AUTOCONTRAST));
    const std::vector<ccmi_tone_op> *kinds[] = {&none, &point, &stats, &sharp, &longest};
    const Geo geos[] = {{nullptr, nullptr, nullptr}, {rects.data(), nullptr, nullptr}, {rects.data(), &rs, nullptr},
                        {nullptr, nullptr, &wp}};
    for (const Geo &g : geos) {
        for (const ccmi_colour *c : {static_cast<const ccmi_colour *>(nullptr), &col})
            for (const ccmi_filter *fl : {static_cast<const ccmi_filter *>(nullptr), &flt}) {
                std::vector<ccmi_frame_geom> geom(n), geom0(n);
                size_t base = 0, need = 0;
                if (plan(b, g, fmt, c, nullptr, fl, geom0, &base) != CCMI_OK) fail("the plan without tone ops");
                {
                    const std::vector<std::vector<ccmi_tone_op>> empty(n);
                    const Tone Z(empty); // every count 0, ops NULL
                    if (plan(b, g, fmt, c, &Z.t, fl, geom, &need) != CCMI_OK || need != base)
                        fail("all counts 0 is not the _flt plan");
                }
                for (int shift = 0; shift < 5; ++shift) { // mixed batches: frame i has kind (i + shift) % 5
                    std::vector<std::vector<ccmi_tone_op>> lists(n);
                    for (int i = 0; i < n; ++i) lists[i] = *kinds[(i + shift) % 5];
                    const Tone T(lists);
                    if (plan(b, g, fmt, c, &T.t, fl, geom, &need) != CCMI_OK) fail("a valid tone list was refused");
                    size_t grow = 0;
                    bool any = false;
                    for (int i = 0; i < n; ++i) any = any || !lists[i].empty();
                    for (int i = 0; i < n && any; ++i) {
                        if (geom[i].width != geom0[i].width || geom[i].height != geom0[i].height) fail("the geometry changed");
                        const size_t frame = r256(12 * (size_t)geom[i].width * geom[i].height);
                        const bool by_filter = fl && (radius[i] > 0 || th[i] <= 1.0f);
                        if (lists[i].empty() && !by_filter) continue;
                        grow += 512;
                        if (!by_filter) grow += frame + 256;
                        int stat = 0;
                        bool sh = false;
                        for (const ccmi_tone_op &o : lists[i]) {
                            sh = sh || o.op == CCMI_TONE_SHARPNESS;
                            stat += o.op == CCMI_TONE_CONTRAST || o.op == CCMI_TONE_AUTOCONTRAST || o.op == CCMI_TONE_EQUALIZE;
                        }
                        grow += (sh ? frame : 0) + 3328 * (size_t)stat;
                    }
                    if (need - base != grow) fail("the workspace does not grow by the documented formula");
                }
            }
        // rejected lists, each in the last frame and in frame 0
        for (int frame : {n - 1, 0}) {
            std::vector<std::vector<ccmi_tone_op>> lists(n, point);
            {
                Tone T(lists);
                T.t.count = nullptr;
                refused(b, g, fmt, T.t, 0);
            }
            {
                Tone T(lists);
                T.t.ops = nullptr;
                refused(b, g, fmt, T.t, 0);
            }
            for (int bad : {-1, CCMI_TONE_MAX_OPS + 1, 0x7fffffff, (int)0x80000000}) {
                Tone T(lists);
                T.count[frame] = bad; // the frames before it keep their counts: nothing past the block is read
                refused(b, g, fmt, T.t, frame);
            }
            for (int bad : {-1, 9, 0x7fffffff}) {
                Tone T(lists);
                T.ops[T.first[frame] + 4].op = bad;
                refused(b, g, fmt, T.t, frame);
            }
            for (int code : {CCMI_TONE_BRIGHTNESS, CCMI_TONE_SATURATION, CCMI_TONE_CONTRAST, CCMI_TONE_SHARPNESS})
                for (float bad : {-0.5f, NAN, INFINITY, -INFINITY}) {
                    Tone T(lists);
                    T.ops[T.first[frame] + 1] = op(code, bad);
                    refused(b, g, fmt, T.t, frame);
                }
            for (int e : {0, 11}) {
                Tone T(lists);
                T.ops[T.first[frame] + 2].v[e] = e ? INFINITY : NAN;
                refused(b, g, fmt, T.t, frame);
            }
            {
                Tone T(lists);
                T.ops[T.first[frame] + 3].v[0] = NAN;
                refused(b, g, fmt, T.t, frame);
            }
            for (float bad : {0.f, 9.f, 2.5f, -1.f, NAN, INFINITY}) {
                Tone T(lists);
                T.ops[T.first[frame] + 1] = op(CCMI_TONE_POSTERIZE, bad);
                refused(b, g, fmt, T.t, frame);
            }
        }
    }
    free(mir);
    free(mat);
    free(counts);
    free(cops);
    free(radius);
    free(th);
    free(taps);
}

} // namespace

int main(int argc, char **argv)
{
    std::vector<std::vector<uint8_t>> all;
    for (int i = 1; i < argc; ++i) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::vector<uint8_t> buf;
        uint8_t tmp[4096];
        for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + k);
        fclose(f);
        all.push_back(buf);
    }
    if (all.empty()) {
        fprintf(stderr, "usage: decode_tone_san stream.cool ...\n");
        return 2;
    }
    // batches of 1, of 5 and of all the streams (repeated to at least 9 frames)
    for (size_t size : {size_t(1), size_t(5), all.size() < 9 ? size_t(9) : all.size()}) {
        Batch b;
        for (size_t i = 0; i < size; ++i) {
            b.sp.push_back(all[i % all.size()].data());
            b.ln.push_back(all[i % all.size()].size());
        }
        if (ccmi_latents_decode(b.sp.data(), b.ln.data(), b.n(), CCMI_LATENT_I16, nullptr, 0, nullptr, 0, nullptr, &b.h) !=
            CCMI_OK)
            fail("a plan-only handle");
        run_batch(b);
        ccmi_latents_free(b.h);
    }
    printf("decode_tone_san: %ld calls, %ld plans succeeded, %ld tone lists refused by all four entry points\n", g_calls, g_ok,
           g_refused);
    return g_ok > 0 && g_refused > 0 ? 0 : 1;
}
