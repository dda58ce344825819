// decode_filter_san.cpp -- stand-alone host program for a sanitizer run of the filter stage's planning
// (ccmi_filter; decode_plan, dec_plan.cpp) on a machine without a GPU, in the form of
// decode_plan_san.cpp.  The plan walks the caller's flat tap array by per-frame offsets, so the radii,
// the taps and the thresholds sit in heap blocks of exactly their sizes (the taps: the sum of r_j + 1
// over the frames with r_j > 0, and no block at all when every radius is 0): a read past an end is
// reported.  Over the streams named on the command line, as streams and as a plan-only latent handle,
// on every geometry (whole frame, regions, a resample, a warp), with and without colour ops: valid
// filters (every radius, mixed batches, solarize alone), every rejected one (radius NULL, a radius out
// of range, taps NULL, a non-finite tap, a NaN threshold), and the run entry points with filters the
// plan rejects or a plan-only handle (refused before any GPU work).  The workspace growth is checked
// against the formula of ccmi.h.  No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_filter_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_latents.hip \
//       -o /tmp/decode_filter_san
//   /tmp/decode_filter_san $(find ../tests/golden/cool -name '*.cool')
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
    fprintf(stderr, "decode_filter_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

// a ccmi_filter whose arrays are heap blocks of exactly their sizes
struct Filter {
    ccmi_filter f{};
    int *radius = nullptr;
    float *taps = nullptr, *th = nullptr;
    int staged = 0;
    Filter(const std::vector<int> &r, const std::vector<float> *thresholds, float tap_scale = 1.f)
    {
        const int n = (int)r.size();
        radius = static_cast<int *>(malloc(sizeof(int) * n));
        size_t nt = 0;
        for (int i = 0; i < n; ++i) {
            radius[i] = r[i];
            if (r[i] > 0 && r[i] <= CCMI_FLT_MAX_RADIUS) nt += (size_t)r[i] + 1;
        }
        if (nt) taps = static_cast<float *>(malloc(sizeof(float) * nt));
        for (size_t k = 0; k < nt; ++k) taps[k] = tap_scale * (float)((k % 7) + 1) / 64.f;
        if (thresholds) {
            th = static_cast<float *>(malloc(sizeof(float) * n));
            for (int i = 0; i < n; ++i) th[i] = (*thresholds)[i];
        }
        for (int i = 0; i < n; ++i) staged += r[i] > 0 || (th && th[i] <= 1.0f);
        f.radius = radius, f.taps = taps, f.solarize = th;
    }
    ~Filter()
    {
        free(radius);
        free(taps);
        free(th);
    }
    Filter(const Filter &) = delete;
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

// both sources' plans of one filter on one geometry; returns the streams' rc, *need its workspace
int plan(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_colour *col, const ccmi_filter *flt,
         std::vector<ccmi_frame_geom> &geom, size_t *need)
{
    const int n = b.n();
    std::vector<ccmi_roi_info> info(n);
    std::vector<ccmi_rect> win(n);
    *need = 0;
    const int rc = ccmi_decode_batch_dev_flt_plan(b.sp.data(), b.ln.data(), n, g.roi, 0, 444, &fmt, g.rs, g.warp, col, flt,
                                                  geom.data(), info.data(), g.warp ? win.data() : nullptr, need);
    ++g_calls;
    size_t need_h = 0;
    std::vector<ccmi_frame_geom> geom_h(n);
    const int rc_h = ccmi_latents_render_flt_plan(b.h, nullptr, n, g.roi, 0, 444, &fmt, g.rs, g.warp, col, flt, geom_h.data(),
                                                  nullptr, nullptr, &need_h);
    ++g_calls;
    if (rc != rc_h) fail("the two sources disagree on a filter");
    if (rc == CCMI_OK) g_ok += 2;
    return rc;
}

// a filter the plan must refuse, naming `frame`: both plans, then both run entry points, which must
// refuse as well before they touch the made-up output pointers
void refused(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_filter &flt, int frame)
{
    const int n = b.n();
    std::vector<ccmi_frame_geom> geom(n);
    size_t need = 0;
    if (plan(b, g, fmt, nullptr, &flt, geom, &need) != CCMI_ERR_ARG) fail("a bad filter was not refused");
    char want[32];
    snprintf(want, sizeof want, "frame %d", frame);
    if (!strstr(ccmi_last_error(), want)) fail("the refusal does not name the frame");
    if (need != 0) fail("a refused plan wrote a workspace size");
    std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
    std::vector<size_t> caps(n, size_t(1) << 30);
    if (ccmi_decode_batch_dev_flt(b.sp.data(), b.ln.data(), n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr,
                                  &flt, 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
        fail("the run entry point took a bad filter");
    if (ccmi_latents_render_flt(b.h, nullptr, n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr, &flt, 0, 444,
                                nullptr, 0, nullptr) != CCMI_ERR_ARG)
        fail("the render entry point ran on a plan-only handle");
    g_calls += 2;
    ++g_refused;
}

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
    ccmi_colour_op *ops = static_cast<ccmi_colour_op *>(calloc(n_ops, sizeof(ccmi_colour_op)));
    for (int i = 0, k = 0; i < n; ++i) {
        ops[k].op = CCMI_COL_BRIGHTNESS, ops[k++].v[0] = 1.1f;
        if (i % 3 == 0) ops[k].op = CCMI_COL_CONTRAST, ops[k++].v[0] = 0.7f;
    }
    const ccmi_colour col{counts, ops};
    const Geo geos[] = {{nullptr, nullptr, nullptr}, {rects.data(), nullptr, nullptr}, {rects.data(), &rs, nullptr},
                        {nullptr, nullptr, &wp}};
    for (const Geo &g : geos) {
        for (const ccmi_colour *c : {static_cast<const ccmi_colour *>(nullptr), &col}) {
            std::vector<ccmi_frame_geom> geom(n), geom0(n);
            size_t base = 0, need = 0;
            if (plan(b, g, fmt, c, nullptr, geom0, &base) != CCMI_OK) fail("the plan without a filter");
            // valid filters: every radius, mixed batches, solarize alone, no frame staged
            std::vector<std::vector<int>> radii;
            std::vector<int> r(n);
            for (int k = 0; k <= CCMI_FLT_MAX_RADIUS; k += 5) {
                for (int i = 0; i < n; ++i) r[i] = (i + k) % (CCMI_FLT_MAX_RADIUS + 1);
                radii.push_back(r);
            }
            radii.push_back(std::vector<int>(n, 0));
            radii.push_back(std::vector<int>(n, CCMI_FLT_MAX_RADIUS));
            std::vector<float> th(n);
            for (int i = 0; i < n; ++i) th[i] = i % 4 == 0 ? 0.5f : i % 4 == 1 ? 2.f : i % 4 == 2 ? 1.f : INFINITY;
            for (const std::vector<int> &rr : radii)
                for (const std::vector<float> *t : {static_cast<const std::vector<float> *>(nullptr),
                                                    static_cast<const std::vector<float> *>(&th)}) {
                    const Filter F(rr, t, -3.5f);
                    if (plan(b, g, fmt, c, &F.f, geom, &need) != CCMI_OK) fail("a valid filter was refused");
                    size_t grow = 0;
                    for (int i = 0; i < n; ++i) {
                        if (geom[i].width != geom0[i].width || geom[i].height != geom0[i].height) fail("the geometry changed");
                        if (rr[i] > 0 || (t && (*t)[i] <= 1.0f))
                            grow += (12 * (size_t)geom[i].width * geom[i].height + 255) / 256 * 256 + 256;
                    }
                    if (need - base != grow) fail("the workspace does not grow by the documented formula");
                }
        }
        // rejected filters, each in the last frame and in frame 0
        for (int frame : {n - 1, 0}) {
            std::vector<int> r(n, 2);
            {
                Filter F(r, nullptr);
                F.f.radius = nullptr;
                refused(b, g, fmt, F.f, 0);
            }
            for (int bad : {-1, CCMI_FLT_MAX_RADIUS + 1, 0x7fffffff, (int)0x80000000}) {
                r.assign(n, 2);
                r[frame] = bad;
                const Filter F(r, nullptr);
                refused(b, g, fmt, F.f, frame);
            }
            {
                r.assign(n, 0);
                r[frame] = 3;
                Filter F(r, nullptr);
                F.f.taps = nullptr;
                refused(b, g, fmt, F.f, frame);
            }
            for (float bad : {NAN, INFINITY, -INFINITY}) {
                r.assign(n, 2);
                r[frame] = CCMI_FLT_MAX_RADIUS;
                const Filter F(r, nullptr);
                F.taps[3 * (size_t)frame + (frame ? CCMI_FLT_MAX_RADIUS : 0)] = bad; // its last tap, or tap 0 of frame 0
                refused(b, g, fmt, F.f, frame);
            }
            {
                std::vector<float> th(n, 0.5f);
                th[frame] = NAN;
                const Filter F(std::vector<int>(n, 0), &th);
                refused(b, g, fmt, F.f, frame);
            }
        }
    }
    free(mir);
    free(mat);
    free(counts);
    free(ops);
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
        fprintf(stderr, "usage: decode_filter_san stream.cool ...\n");
        return 2;
    }
    // batches of 1, of 5 and of all the streams (repeated to at least 9 frames)
    for (size_t size : {size_t(1), size_t(5), all.size() < 9 ? size_t(9) : all.size()}) {
        Batch b;
        for (size_t i = 0; i < size; ++i) {
            b.sp.push_back(all[i % all.size()].data());
            b.ln.push_back(all[i % all.size()].size());
        }
        if (ccmi_latents_decode(b.sp.data(), b.ln.data(), b.n(), CCMI_LATENT_I16, nullptr, 0, nullptr, 0, nullptr, &b.h) != CCMI_OK)
            fail("a plan-only handle");
        run_batch(b);
        ccmi_latents_free(b.h);
    }
    printf("decode_filter_san: %ld calls, %ld plans succeeded, %ld filters refused by all four entry points\n", g_calls, g_ok,
           g_refused);
    return g_ok > 0 && g_refused > 0 ? 0 : 1;
}
