// decode_mix_san.cpp -- stand-alone host program for a sanitizer run of the mix stage's planning
// (ccmi_mix; decode_plan, dec_plan.cpp) on a machine without a GPU, in the form of decode_tone_san.cpp.
// The plan walks the caller's flat rectangle array by per-frame counts and reads seed, partner, lam and
// box per frame, so every array of a ccmi_mix sits in a heap block of exactly its size (no block at all
// for a NULL member): a read past an end is reported.  Over the streams named on the command line, as
// streams and as a plan-only latent handle, on every geometry (whole frames, regions of one size, a
// resample, a warp), with and without colour ops, tone ops and a filter: valid batches (untouched
// frames, constant and noise rectangles, the longest list, blends, boxes, partners of themselves,
// partner-only frames), every rejected one (a count out of range, rects NULL, a non-finite value or
// sigma, a negative sigma, a negative size, a rectangle or box outside the frame, a partner outside the
// call or of another size, lam NULL, NaN or outside [0, 1]), and the run entry points with arguments the
// plan rejects or a plan-only handle (refused before any GPU work).  The workspace growth is checked
// against the formula of ccmi.h.  No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_mix_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_tone.hip \
//       csrc/dec_mix.hip csrc/dec_latents.hip -o /tmp/decode_mix_san
//   /tmp/decode_mix_san $(find ../tests/golden/cool -name '*.cool')
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
    fprintf(stderr, "decode_mix_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

ccmi_erase_rect rect(int x, int y, int w, int h, float v, float sigma = 0.f)
{
    return ccmi_erase_rect{x, y, w, h, {v, -v, 0.5f * v}, sigma};
}

template <typename T> T *block(const std::vector<T> &v)
{
    if (v.empty()) return nullptr;
    T *p = static_cast<T *>(malloc(sizeof(T) * v.size()));
    memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

// a ccmi_mix whose arrays are heap blocks of exactly their sizes; an empty vector is a NULL member
struct Mix {
    ccmi_mix m{};
    int *count, *partner;
    ccmi_erase_rect *rects;
    uint64_t *seed;
    float *lam;
    ccmi_rect *box;
    std::vector<size_t> first; // frame j's first rectangle in the flat array
    Mix(const std::vector<std::vector<ccmi_erase_rect>> &lists, const std::vector<int> &partners, const std::vector<float> &lams,
        const std::vector<ccmi_rect> &boxes, const std::vector<uint64_t> &seeds)
    {
        std::vector<int> counts;
        std::vector<ccmi_erase_rect> flat;
        for (const auto &l : lists) {
            first.push_back(flat.size());
            counts.push_back((int)l.size());
            flat.insert(flat.end(), l.begin(), l.end());
        }
        count = block(counts), rects = block(flat), partner = block(partners), lam = block(lams), box = block(boxes), seed = block(seeds);
        m.count = count, m.rects = rects, m.seed = seed, m.partner = partner, m.lam = lam, m.box = box;
    }
    ~Mix()
    {
        free(count), free(rects), free(partner), free(lam), free(box), free(seed);
    }
    Mix(const Mix &) = delete;
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

// both sources' plans of one mix on one geometry; returns the streams' rc, *need its workspace
int plan(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_colour *col, const ccmi_tone *tone,
         const ccmi_filter *flt, const ccmi_mix *mix, std::vector<ccmi_frame_geom> &geom, size_t *need)
{
    const int n = b.n();
    std::vector<ccmi_roi_info> info(n);
    std::vector<ccmi_rect> win(n);
    *need = 0;
    const int rc = ccmi_decode_batch_dev_mix_plan(b.sp.data(), b.ln.data(), n, g.roi, 0, 444, &fmt, g.rs, g.warp, col, tone, flt,
                                                  mix, geom.data(), info.data(), g.warp ? win.data() : nullptr, need);
    ++g_calls;
    size_t need_h = 0;
    std::vector<ccmi_frame_geom> geom_h(n);
    const int rc_h = ccmi_latents_render_mix_plan(b.h, nullptr, n, g.roi, 0, 444, &fmt, g.rs, g.warp, col, tone, flt, mix,
                                                  geom_h.data(), nullptr, nullptr, &need_h);
    ++g_calls;
    if (rc != rc_h) fail("the two sources disagree on a mix");
    if (rc == CCMI_OK) g_ok += 2;
    return rc;
}

// a mix the plan must refuse, naming `frame`: both plans, then both run entry points, which must refuse
// as well before they touch the made-up output pointers
void refused(const Batch &b, const Geo &g, const ccmi_tensor_fmt &fmt, const ccmi_mix &mix, int frame)
{
    const int n = b.n();
    std::vector<ccmi_frame_geom> geom(n);
    size_t need = 0;
    if (plan(b, g, fmt, nullptr, nullptr, nullptr, &mix, geom, &need) != CCMI_ERR_ARG) fail("a bad mix was not refused");
    char want[32];
    snprintf(want, sizeof want, "frame %d:", frame);
    if (!strstr(ccmi_last_error(), want)) fail("the refusal does not name the frame");
    if (need != 0) fail("a refused plan wrote a workspace size");
    std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
    std::vector<size_t> caps(n, size_t(1) << 30);
    if (ccmi_decode_batch_dev_mix(b.sp.data(), b.ln.data(), n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr,
                                  nullptr, nullptr, &mix, 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
        fail("the run entry point took a bad mix");
    if (ccmi_latents_render_mix(b.h, nullptr, n, g.roi, outs.data(), caps.data(), &fmt, g.rs, g.warp, nullptr, nullptr, nullptr,
                                &mix, 0, 444, nullptr, 0, nullptr) != CCMI_ERR_ARG)
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
    int *ccounts = static_cast<int *>(malloc(sizeof(int) * n));
    for (int i = 0; i < n; ++i) ccounts[i] = 1;
    ccmi_colour_op *cops = static_cast<ccmi_colour_op *>(calloc(n, sizeof(ccmi_colour_op)));
    for (int i = 0; i < n; ++i) cops[i].op = i % 3 ? CCMI_COL_BRIGHTNESS : CCMI_COL_CONTRAST, cops[i].v[0] = 1.1f;
    const ccmi_colour col{ccounts, cops};
    // a filter that blurs every fourth frame and solarizes every fourth + 1; tone ops on every third frame
    int *radius = static_cast<int *>(malloc(sizeof(int) * n));
    float *th = static_cast<float *>(malloc(sizeof(float) * n));
    int n_blur = 0;
    for (int i = 0; i < n; ++i) n_blur += (radius[i] = i % 4 == 0 ? 2 : 0) > 0, th[i] = i % 4 == 1 ? 0.5f : 2.f;
    float *taps = static_cast<float *>(malloc(sizeof(float) * 3 * (n_blur ? n_blur : 1)));
    for (int k = 0; k < 3 * n_blur; ++k) taps[k] = 0.2f;
    const ccmi_filter flt{radius, taps, th};
    int *zero_radius = static_cast<int *>(calloc(n, sizeof(int)));
    int *tcount = static_cast<int *>(malloc(sizeof(int) * n));
    int n_tone = 0;
    for (int i = 0; i < n; ++i) n_tone += tcount[i] = i % 3 == 2 ? 2 : 0;
    ccmi_tone_op *tops = n_tone ? static_cast<ccmi_tone_op *>(calloc(n_tone, sizeof(ccmi_tone_op))) : nullptr;
    for (int k = 0; k < n_tone; ++k) tops[k].op = k & 1 ? CCMI_TONE_EQUALIZE : CCMI_TONE_SHARPNESS, tops[k].v[0] = 1.5f;
    const ccmi_tone tone{tcount, tops};

    // the stored size is 33 x 17 (regions), 29 x 13 (resample, warp) or the frame's own
    const Geo geos[] = {{same.data(), nullptr, nullptr}, {rects.data(), &rs, nullptr}, {nullptr, nullptr, &wp}, {nullptr, nullptr, nullptr}};
    for (const Geo &g : geos) {
        const bool whole = !g.roi && !g.warp; // frames of their own sizes: a frame's only legal partner may be itself
        for (const ccmi_colour *c : {static_cast<const ccmi_colour *>(nullptr), &col})
            for (const ccmi_tone *tn : {static_cast<const ccmi_tone *>(nullptr), &tone})
                for (const ccmi_filter *fl : {static_cast<const ccmi_filter *>(nullptr), &flt}) {
                    std::vector<ccmi_frame_geom> geom(n), geom0(n);
                    size_t plain = 0, need = 0;
                    if (plan(b, g, fmt, c, tn, fl, nullptr, geom0, &plain) != CCMI_OK) fail("the plan without a mix");
                    {
                        const Mix Z(std::vector<std::vector<ccmi_erase_rect>>(n), std::vector<int>(n, -1), {}, {}, {});
                        const Mix N({}, {}, {}, {}, {}); // every member NULL
                        if (plan(b, g, fmt, c, tn, fl, &Z.m, geom, &need) != CCMI_OK || need != plain) fail("an idle mix is not the _tone plan");
                        if (plan(b, g, fmt, c, tn, fl, &N.m, geom, &need) != CCMI_OK || need != plain) fail("a NULL mix is not the _tone plan");
                    }
                    for (int shift = 0; shift < 5; ++shift) { // frame i has kind (i + shift) % 5
                        std::vector<std::vector<ccmi_erase_rect>> lists(n);
                        std::vector<int> partners(n, -1);
                        std::vector<float> lams(n, 0.25f);
                        std::vector<ccmi_rect> boxes(n, ccmi_rect{0, 0, 0, 0});
                        std::vector<uint64_t> seeds(n);
                        std::vector<char> staged(n, 0);
                        for (int i = 0; i < n; ++i) {
                            const int w = geom0[i].width, h = geom0[i].height;
                            seeds[i] = 0x8000000000000005ull + (uint64_t)i;
                            switch ((i + shift) % 5) {
                            case 1: lists[i] = {rect(1, 2, 5, 4, 0.5f)}; break;
                            case 2: // the longest list: the whole frame, the last pixel, an empty one, noise
                                lists[i] = {rect(0, 0, w, h, 1.f), rect(w - 1, h - 1, 1, 1, 2.f), rect(-9, 99999, 0, 7, 3.f), rect(2, 1, 3, 3, 0.f, 1.f)};
                                break;
                            case 3: partners[i] = whole ? i : (i + 1) % n; break;
                            case 4: partners[i] = i, boxes[i] = ccmi_rect{w - 2, h - 1, 2, 1}; break;
                            default: break;
                            }
                            if (!lists[i].empty() || partners[i] >= 0) staged[i] = 1;
                            if (partners[i] >= 0) staged[partners[i]] = 1;
                        }
                        for (int i = 0; i < n; ++i) // an earlier frame's partner stages a later frame as well
                            if (partners[i] >= 0) staged[partners[i]] = 1;
                        const Mix X(lists, partners, lams, boxes, seeds);
                        if (plan(b, g, fmt, c, tn, fl, &X.m, geom, &need) != CCMI_OK) fail("a valid mix was refused");
                        // the base: the _tone call in which the staged frames take the filter stage as well
                        std::vector<float> bth(n);
                        size_t grow = 0;
                        bool any = false;
                        for (int i = 0; i < n; ++i) {
                            const bool by_filter = fl && (radius[i] > 0 || th[i] <= 1.0f);
                            bth[i] = staged[i] && !by_filter ? 1.0f : fl ? th[i] : 2.f;
                            any = any || staged[i];
                            if (!staged[i]) continue;
                            if (geom[i].width != geom0[i].width || geom[i].height != geom0[i].height) fail("the geometry changed");
                            grow += 256 + (by_filter ? r256(12 * (size_t)geom[i].width * geom[i].height) : 0);
                        }
                        const ccmi_filter bflt{fl ? radius : zero_radius, fl ? taps : nullptr, bth.data()};
                        size_t base = 0;
                        if (plan(b, g, fmt, c, tn, any ? &bflt : fl, nullptr, geom, &base) != CCMI_OK) fail("the base plan");
                        if (need - base != grow) fail("the workspace does not grow by the documented formula");
                    }
                }
        // rejected ones, each in the last frame and in frame 0
        for (int frame : {n - 1, 0}) {
            std::vector<ccmi_frame_geom> geom0(n);
            size_t plain = 0;
            if (plan(b, g, fmt, nullptr, nullptr, nullptr, nullptr, geom0, &plain) != CCMI_OK) fail("the plan without a mix");
            const int w = geom0[frame].width, h = geom0[frame].height;
            const std::vector<std::vector<ccmi_erase_rect>> lists(n, {rect(1, 1, 2, 2, 0.5f), rect(0, 0, 1, 1, 1.f, 0.5f)});
            const std::vector<int> self = [&] {
                std::vector<int> p(n);
                for (int i = 0; i < n; ++i) p[i] = i;
                return p;
            }();
            const std::vector<float> lams(n, 0.5f);
            const std::vector<ccmi_rect> none(n, ccmi_rect{0, 0, 0, 0});
            for (int bad : {-1, CCMI_MIX_MAX_RECTS + 1, INT_MAX, INT_MIN}) {
                Mix X(lists, {}, {}, {}, {});
                X.count[frame] = bad; // the frames before it keep their counts: nothing past the block is read
                refused(b, g, fmt, X.m, frame);
            }
            {
                Mix X(lists, {}, {}, {}, {});
                X.m.rects = nullptr;
                refused(b, g, fmt, X.m, 0);
            }
            for (int e = 0; e < 3; ++e)
                for (float bad : {NAN, INFINITY, -INFINITY}) {
                    Mix X(lists, {}, {}, {}, {});
                    X.rects[X.first[frame] + 1].v[e] = bad;
                    refused(b, g, fmt, X.m, frame);
                }
            for (float bad : {NAN, INFINITY, -INFINITY, -0.5f}) {
                Mix X(lists, {}, {}, {}, {});
                X.rects[X.first[frame]].sigma = bad;
                refused(b, g, fmt, X.m, frame);
            }
            const ccmi_rect outside[] = {{0, 0, -1, 2}, {0, 0, 2, -1}, {-1, 0, 2, 2}, {0, -1, 2, 2}, {w - 1, 0, 2, 1}, {0, h - 1, 1, 2},
                                         {0, 0, w + 1, 1}, {0, 0, 1, h + 1}, {w, 0, 1, 1}, {INT_MAX, 0, 2, 1}, {0, INT_MAX, 1, 2},
                                         {0, 0, INT_MAX, INT_MAX}};
            for (const ccmi_rect &q : outside) {
                Mix X(lists, {}, {}, {}, {});
                ccmi_erase_rect &r = X.rects[X.first[frame] + 1];
                r.x = q.x, r.y = q.y, r.w = q.w, r.h = q.h;
                refused(b, g, fmt, X.m, frame);
                Mix Y({}, self, lams, none, {});
                Y.box[frame] = q;
                refused(b, g, fmt, Y.m, frame);
            }
            for (int bad : {-2, n, INT_MAX, INT_MIN}) {
                Mix X({}, self, lams, {}, {});
                X.partner[frame] = bad;
                refused(b, g, fmt, X.m, frame);
            }
            {
                Mix X({}, self, {}, {}, {}); // lam NULL where every frame blends
                refused(b, g, fmt, X.m, 0);
            }
            for (float bad : {NAN, -0.25f, 1.5f, INFINITY, -INFINITY}) {
                Mix X({}, self, lams, none, {});
                X.lam[frame] = bad;
                refused(b, g, fmt, X.m, frame);
            }
            // a partner of another stored size: whole frames of different streams
            for (int p = 0; p < n; ++p)
                if (geom0[p].width != w || geom0[p].height != h) {
                    Mix X({}, self, lams, {}, {});
                    X.partner[frame] = p;
                    refused(b, g, fmt, X.m, frame);
                    break;
                }
        }
    }
    free(mir), free(mat), free(ccounts), free(cops), free(radius), free(th), free(taps), free(zero_radius), free(tcount), free(tops);
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
        fprintf(stderr, "usage: decode_mix_san stream.cool ...\n");
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
    printf("decode_mix_san: %ld calls, %ld plans succeeded, %ld mixes refused by all four entry points\n", g_calls, g_ok, g_refused);
    return g_ok > 0 && g_refused > 0 ? 0 : 1;
}
