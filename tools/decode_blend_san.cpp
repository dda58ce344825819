// decode_blend_san.cpp -- stand-alone host program for a sanitizer run of the blend stage's planning
// (ccmi_blend; decode_plan, dec_plan.cpp) on a machine without a GPU, in the form of decode_mix_san.cpp.
// The plan walks the caller's flat source and weight arrays by per-frame counts and reads silent per frame,
// so every array of a ccmi_blend sits in a heap block of exactly its size (no block at all for a NULL
// member): a read past an end is reported.  Over the streams named on the command line, as streams and as a
// plan-only latent handle, on every geometry with one stored size (regions of one size, a resample, a warp)
// and on whole frames, with and without a mix and a filter: valid batches (idle blends, the identity, the
// longest list, a source twice, silent sources, silent frames nobody reads, blended partners), every
// rejected one (a count out of range, source or weight NULL, a source outside the call or of another size, a
// weight that is not finite, a silent frame with terms, rectangles or a partner, a non-silent frame without
// an output), and the run entry points with arguments the plan rejects or a plan-only handle (refused before
// any GPU work).  The workspace growth is checked against the formula of ccmi.h.  No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_blend_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_tone.hip \
//       csrc/dec_mix.hip csrc/dec_blend.hip csrc/dec_latents.hip -o /tmp/decode_blend_san
//   /tmp/decode_blend_san $(find ../tests/golden/cool -name '*.cool')
#include <limits.h>
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
    fprintf(stderr, "decode_blend_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

template <typename T> T *block(const std::vector<T> &v)
{
    if (v.empty()) return nullptr;
    T *p = static_cast<T *>(malloc(sizeof(T) * v.size()));
    memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

struct Term {
    int source;
    float weight;
};

// a ccmi_blend whose arrays are heap blocks of exactly their sizes; an empty vector is a NULL member
struct Blend {
    ccmi_blend b{};
    int *count, *source, *silent;
    float *weight;
    std::vector<size_t> first; // frame j's first term in the flat arrays
    Blend(const std::vector<std::vector<Term>> &lists, const std::vector<int> &silents)
    {
        std::vector<int> counts, sources;
        std::vector<float> weights;
        for (const auto &l : lists) {
            first.push_back(sources.size());
            counts.push_back((int)l.size());
            for (const Term &t : l) sources.push_back(t.source), weights.push_back(t.weight);
        }
        count = block(counts), source = block(sources), weight = block(weights), silent = block(silents);
        b.count = count, b.source = source, b.weight = weight, b.silent = silent;
    }
    ~Blend() { free(count), free(source), free(weight), free(silent); }
    Blend(const Blend &) = delete;
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

// both sources' plans of one blend on one geometry; returns the streams' rc, *need its workspace
int plan(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_filter *flt, const ccmi_blend *blend,
         const ccmi_mix *mix, std::vector<ccmi_frame_geom> &geom, size_t *need)
{
    const int n = b.n();
    std::vector<ccmi_roi_info> info(n);
    std::vector<ccmi_rect> win(n);
    *need = 0;
    const int rc = ccmi_decode_batch_dev_blend_plan(b.sp.data(), b.ln.data(), n, g.roi, 0, 444, &fmt, g.rs, g.warp, nullptr, nullptr,
                                                    flt, blend, mix, geom.data(), info.data(), g.warp ? win.data() : nullptr, need);
    ++g_calls;
    size_t need_h = 0;
    std::vector<ccmi_frame_geom> geom_h(n);
    const int rc_h = ccmi_latents_render_blend_plan(b.h, nullptr, n, g.roi, 0, 444, &fmt, g.rs, g.warp, nullptr, nullptr, flt, blend,
                                                    mix, geom_h.data(), nullptr, nullptr, &need_h);
    ++g_calls;
    if (rc != rc_h) fail("the two sources disagree on a blend");
    if (rc == CCMI_OK) g_ok += 2;
    return rc;
}

// a blend the plan must refuse, naming `frame`: both plans, then both run entry points, which must refuse
// as well before they touch the made-up output pointers
void refused(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_blend &blend, const ccmi_mix *mix, int frame)
{
    const int n = b.n();
    std::vector<ccmi_frame_geom> geom(n);
    size_t need = 0;
    if (plan(b, g, fmt, nullptr, &blend, mix, geom, &need) != CCMI_ERR_ARG) fail("a bad blend was not refused");
    char want[32];
    snprintf(want, sizeof want, "frame %d:", frame);
    if (!strstr(ccmi_last_error(), want)) fail("the refusal does not name the frame");
    if (need != 0) fail("a refused plan wrote a workspace size");
    std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
    std::vector<size_t> caps(n, size_t(1) << 30);
    if (ccmi_decode_batch_dev_blend(b.sp.data(), b.ln.data(), n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr,
                                    nullptr, nullptr, &blend, mix, 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
        fail("the run entry point took a bad blend");
    if (ccmi_latents_render_blend(b.h, nullptr, n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr, nullptr, nullptr,
                                  &blend, mix, 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
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
    std::vector<ccmi_rect> same(n), rects(n);
    for (int i = 0; i < n; ++i) same[i] = ccmi_rect{2 * (i % 3), 4, 33, 17}, rects[i] = ccmi_rect{2 * (i % 3), 4, 33 + 2 * (i % 5), 17 + (i % 4)};
    const ccmi_resample rs{29, 13, CCMI_FILTER_TRIANGLE};
    float *mat = static_cast<float *>(malloc(sizeof(float) * 6 * n));
    for (int i = 0; i < n; ++i) {
        const float m[6] = {0.5f, 0.1f * (float)(i % 3), 3.f, -0.1f, 0.5f, 2.f};
        memcpy(mat + 6 * i, m, sizeof m);
    }
    ccmi_warp wp{};
    wp.out_w = 29, wp.out_h = 13, wp.pad = CCMI_PAD_EDGE, wp.matrix = mat;
    // a filter that blurs every fourth frame and solarizes every fourth + 1
    int *radius = static_cast<int *>(malloc(sizeof(int) * n));
    float *th = static_cast<float *>(malloc(sizeof(float) * n));
    int n_blur = 0;
    for (int i = 0; i < n; ++i) n_blur += (radius[i] = i % 4 == 0 ? 2 : 0) > 0, th[i] = i % 4 == 1 ? 0.5f : 2.f;
    float *taps = static_cast<float *>(malloc(sizeof(float) * 3 * (n_blur ? n_blur : 1)));
    for (int k = 0; k < 3 * n_blur; ++k) taps[k] = 0.2f;
    const ccmi_filter flt{radius, taps, th};
    // lam 1 for every frame: a frame that is its own MixUp partner is mix-staged and nothing else
    float *ones = static_cast<float *>(malloc(sizeof(float) * n));
    for (int i = 0; i < n; ++i) ones[i] = 1.f;

    // one stored size per call: 33 x 17 (regions) or 29 x 13 (resample, warp); then whole frames of their own sizes
    const Geo geos[] = {{same.data(), nullptr, nullptr}, {rects.data(), &rs, nullptr}, {nullptr, nullptr, &wp}, {nullptr, nullptr, nullptr}};
    for (const Geo &g : geos) {
        const bool whole = !g.roi && !g.warp; // a frame's only legal source may be itself
        for (const ccmi_filter *fl : {static_cast<const ccmi_filter *>(nullptr), &flt}) {
            std::vector<ccmi_frame_geom> geom(n), geom0(n);
            size_t plain = 0, need = 0;
            if (plan(b, g, fmt, fl, nullptr, nullptr, geom0, &plain) != CCMI_OK) fail("the plan without a blend");
            {
                const Blend Z(std::vector<std::vector<Term>>(n), std::vector<int>(n, 0));
                const Blend N({}, {}); // every member NULL
                if (plan(b, g, fmt, fl, &Z.b, nullptr, geom, &need) != CCMI_OK || need != plain) fail("an idle blend is not the _mix plan");
                if (plan(b, g, fmt, fl, &N.b, nullptr, geom, &need) != CCMI_OK || need != plain) fail("a NULL blend is not the _mix plan");
            }
            for (int shift = 0; shift < 5; ++shift) { // frame i has kind (i + shift) % 5
                std::vector<std::vector<Term>> lists(n);
                std::vector<int> silents(n, 0), partners(n, -1);
                std::vector<char> staged(n, 0);
                for (int i = 0; i < n; ++i) {
                    const int other = whole ? i : (i + 1) % n;
                    switch ((i + shift) % 5) {
                    case 1: lists[i] = {{i, 1.f}}; break; // the identity
                    case 2: // the longest list: itself, a source twice, weights 0, negative and huge
                        lists[i] = {{i, 0.f}, {other, -2.5f}, {other, 3e38f}, {i, 1.f}, {other, -0.f}, {i, 0.125f}, {other, 0.5f}, {i, 1e-30f}};
                        break;
                    case 3: silents[i] = 1; break; // a silent frame, read by the frame before it or by nobody
                    case 4: lists[i] = {{other, 0.5f}, {i, 0.5f}}, partners[i] = i; break; // and MixUp with itself
                    default: break;
                    }
                }
                for (int i = 0; i < n; ++i) {
                    if (!lists[i].empty() || silents[i] || partners[i] >= 0) staged[i] = 1;
                    for (const Term &t : lists[i]) staged[t.source] = 1;
                }
                for (int i = 0; i < n; ++i) // a silent frame has neither terms nor a partner
                    if (silents[i]) lists[i].clear(), partners[i] = -1;
                const Blend X(lists, silents);
                ccmi_mix mx{};
                int *pp = block(partners);
                mx.partner = pp, mx.lam = ones;
                if (plan(b, g, fmt, fl, &X.b, &mx, geom, &need) != CCMI_OK) fail("a valid blend was refused");
                // the base: the _mix call that mix-stages the same frames, each its own partner with lam 1
                std::vector<int> bp(n, -1);
                int m = 0;
                for (int i = 0; i < n; ++i)
                    if (staged[i]) bp[i] = i, ++m;
                ccmi_mix base_mix{};
                base_mix.partner = bp.data(), base_mix.lam = ones;
                size_t base = 0;
                if (plan(b, g, fmt, fl, nullptr, m ? &base_mix : nullptr, geom, &base) != CCMI_OK) fail("the base plan");
                if (need - base != (m ? r256(64 * (size_t)m) : 0)) fail("the workspace does not grow by the documented formula");
                for (int i = 0; i < n; ++i)
                    if (geom[i].width != geom0[i].width || geom[i].height != geom0[i].height) fail("the geometry changed");
                free(pp);
            }
        }
        // rejected ones, each in the last frame and in frame 0
        for (int frame : {n - 1, 0}) {
            std::vector<ccmi_frame_geom> geom0(n);
            size_t plain = 0;
            if (plan(b, g, fmt, nullptr, nullptr, nullptr, geom0, &plain) != CCMI_OK) fail("the plan without a blend");
            const int w = geom0[frame].width, h = geom0[frame].height;
            std::vector<std::vector<Term>> lists(n);
            for (int i = 0; i < n; ++i) lists[i] = {{i, 0.5f}, {i, 0.5f}};
            for (int bad : {-1, CCMI_BLEND_MAX_TERMS + 1, INT_MAX, INT_MIN}) {
                Blend X(lists, {});
                X.count[frame] = bad; // the frames before it keep their counts: nothing past the blocks is read
                refused(b, g, fmt, X.b, nullptr, frame);
            }
            {
                Blend X(lists, {});
                X.b.source = nullptr;
                refused(b, g, fmt, X.b, nullptr, 0);
                Blend Y(lists, {});
                Y.b.weight = nullptr;
                refused(b, g, fmt, Y.b, nullptr, 0);
            }
            for (int bad : {-1, n, INT_MAX, INT_MIN}) {
                Blend X(lists, {});
                X.source[X.first[frame] + 1] = bad;
                refused(b, g, fmt, X.b, nullptr, frame);
            }
            for (float bad : {NAN, INFINITY, -INFINITY}) {
                Blend X(lists, {});
                X.weight[X.first[frame] + 1] = bad;
                refused(b, g, fmt, X.b, nullptr, frame);
            }
            { // a silent frame with terms, with a rectangle, with a partner
                std::vector<int> silents(n, 0);
                silents[frame] = 1;
                Blend X(lists, silents);
                refused(b, g, fmt, X.b, nullptr, frame);
                std::vector<std::vector<Term>> none(n);
                Blend Y(none, silents);
                std::vector<int> counts(n, 0), partners(n, -1);
                counts[frame] = 1;
                const ccmi_erase_rect r{0, 0, 1, 1, {0.f, 0.f, 0.f}, 0.f};
                ccmi_mix er{};
                er.count = counts.data(), er.rects = &r;
                refused(b, g, fmt, Y.b, &er, frame);
                partners[frame] = frame;
                ccmi_mix pm{};
                pm.partner = partners.data(), pm.lam = ones;
                refused(b, g, fmt, Y.b, &pm, frame);
                // alone it is fine, and the run refuses a non-silent frame without an output, not the silent one
                std::vector<ccmi_frame_geom> geom(n);
                size_t need = 0;
                if (plan(b, g, fmt, nullptr, &Y.b, nullptr, geom, &need) != CCMI_OK) fail("a silent frame nobody reads was refused");
                if (n > 1) { // (a call of one silent frame would be accepted and run)
                    std::vector<void *> outs(n, nullptr);
                    std::vector<size_t> caps(n, 0);
                    const int rc = ccmi_decode_batch_dev_blend(b.sp.data(), b.ln.data(), n, g.roi, outs.data(), caps.data(), &fmt, g.rs,
                                                               g.warp, nullptr, nullptr, nullptr, &Y.b, nullptr, 0, 444, nullptr, 0, nullptr);
                    ++g_calls;
                    char want[32];
                    snprintf(want, sizeof want, "output %d ", frame == 0 ? 1 : 0);
                    if (rc != CCMI_ERR_ARG || !strstr(ccmi_last_error(), want)) fail("a NULL output of a non-silent frame");
                }
            }
            // a source of another stored size: whole frames of different streams
            for (int p = 0; p < n; ++p)
                if (geom0[p].width != w || geom0[p].height != h) {
                    Blend X(lists, {});
                    X.source[X.first[frame]] = p;
                    refused(b, g, fmt, X.b, nullptr, frame);
                    break;
                }
        }
    }
    free(mat), free(radius), free(th), free(taps), free(ones);
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
        fprintf(stderr, "usage: decode_blend_san stream.cool ...\n");
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
    printf("decode_blend_san: %ld calls, %ld plans succeeded, %ld blends refused by all four entry points\n", g_calls, g_ok, g_refused);
    return g_ok > 0 && g_refused > 0 ? 0 : 1;
}
