// decode_plan_san.cpp -- stand-alone host program for a sanitizer run of the decoder's planner
// (decode_plan, dec_plan.cpp) on a machine without a GPU: every header-only entry point, the
// latent store's layout and plan-only handles (ccmi_latents_*, store = NULL) with their render
// planning included, the formatted sinks (ccmi_tensor_fmt: element types, stride sets, a mirror
// array of exactly n bytes, and the run entry point with capacities it must reject), the resampling
// sinks (ccmi_resample: output sizes in and out of range, an unknown filter), the colouring sinks
// (ccmi_colour: counts and ops in heap blocks of exactly their sizes, every plan error), the warping sinks
// (ccmi_warp: sizes in and out of range, non-finite entries, the 2^22 bound, matrices that put the
// output wholly outside the frame, singular matrices; the matrices sit in a heap block of exactly
// 6 n floats and the windows in one of exactly n rects), over the streams named on the command line, whole, in batches of 7, over a list of regions, and
// truncated at each length from 0 to the header size plus 8.  Every (truncated) stream sits in
// a heap block of exactly its length, so a read past its end is reported.  No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_plan_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_tone.hip \
//       csrc/dec_mix.hip csrc/dec_latents.hip -o /tmp/decode_plan_san
//   /tmp/decode_plan_san $(find ../tests/golden/cool ../tests/golden/cool_synth -name '*.cool')
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../cool-chic_amd/csrc/ccmi_internal.h"

// the float forward path is not linked: ccmi_api.cpp only needs the symbols
int ccmi_launch_arm_f32(const ccmi_arm_args *, hipStream_t, int) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_ups_f32(const ccmi_ups_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_syn_f32(const ccmi_syn_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_post_f32(const ccmi_post_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }

namespace {

struct Stream {
    uint8_t *p;
    size_t n;
};

Stream exact_copy(const uint8_t *src, size_t n)
{
    uint8_t *p = static_cast<uint8_t *>(malloc(n ? n : 1));
    if (n) memcpy(p, src, n);
    return Stream{p, n};
}

long g_calls = 0, g_ok = 0;

void count(int rc)
{
    ++g_calls;
    if (rc == CCMI_OK) ++g_ok;
}

// every header-only entry point on one batch; rects: one per stream
void plan_all(const std::vector<Stream> &b, const std::vector<ccmi_rect> &rects, int bd, int chroma)
{
    const int n = (int)b.size();
    std::vector<const uint8_t *> sp(n);
    std::vector<size_t> ln(n), sizes(n);
    for (int i = 0; i < n; ++i) sp[i] = b[i].p, ln[i] = b[i].n;
    std::vector<ccmi_frame_geom> geom(n);
    std::vector<ccmi_roi_info> info(n);
    size_t need = 0;
    for (int yuv = 0; yuv < 2; ++yuv) {
        count(ccmi_decode_output_size(sp[0], ln[0], bd, chroma, yuv, &need));
        count(ccmi_decode_batch_workspace_bytes(sp.data(), ln.data(), n, bd, chroma, yuv, &need));
        count(ccmi_decode_batch_plan(sp.data(), ln.data(), n, bd, chroma, yuv, sizes.data(), &need));
    }
    for (int sample = 0; sample < 3; ++sample) {
        count(ccmi_decode_batch_dev_plan(sp.data(), ln.data(), n, bd, chroma, sample, geom.data(), &need));
        count(ccmi_decode_batch_dev_roi_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, sample, geom.data(),
                                             info.data(), &need));
        count(ccmi_decode_batch_dev_roi_plan(sp.data(), ln.data(), n, nullptr, bd, chroma, sample, geom.data(), nullptr,
                                             &need));
    }
    // the formatted sink: every element type (one unknown), stride sets that are planar, NHWC,
    // padded, aliasing and negative; the mirror flags sit in a heap block of exactly n bytes
    uint8_t *mir = static_cast<uint8_t *>(malloc(n));
    for (int i = 0; i < n; ++i) mir[i] = (uint8_t)(i & 1);
    const int64_t strides[][3] = {{0, 0, 0}, {1, 3 * 4096, 3}, {1 << 24, 4100, 1}, {1, 1, 1}, {7, -1, 1}, {0, 16, 1}};
    std::vector<ccmi_tensor_fmt> fmts;
    for (int elem = 0; elem < 4; ++elem)
        for (const auto &st : strides) {
            ccmi_tensor_fmt f{};
            f.elem = elem, f.colour = elem & 1;
            for (int c = 0; c < 3; ++c) f.scale[c] = 4.f + c, f.bias[c] = -1.f;
            f.stride_c = st[0], f.stride_y = st[1], f.stride_x = st[2];
            f.mirror = elem == 2 ? nullptr : mir;
            fmts.push_back(f);
        }
    fmts.back().scale[1] = 1.f / 0.f; // non-finite
    fmts[0].colour = 2;               // unknown
    for (const ccmi_tensor_fmt &f : fmts) {
        count(ccmi_decode_batch_dev_fmt_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &f, geom.data(), info.data(),
                                             &need));
        count(ccmi_decode_batch_dev_fmt_plan(sp.data(), ln.data(), n, nullptr, bd, chroma, &f, geom.data(), nullptr, &need));
    }
    // the resampling sink: output sizes in and out of range, an unknown filter, over the first
    // stride sets of every element type; rs NULL is the formatted plan itself
    const ccmi_resample sizes_rs[] = {{224, 224, 0}, {1, 1, 0}, {16384, 3, 0}, {7, 16384, 0}, {0, 8, 0},
                                      {8, -1, 0},    {16385, 8, 0}, {0x7fffffff, 0x7fffffff, 0}, {8, 8, 1}};
    for (const ccmi_resample &rs : sizes_rs)
        for (size_t k = 0; k < fmts.size(); k += 5) {
            count(ccmi_decode_batch_dev_rs_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &fmts[k], &rs, geom.data(),
                                                info.data(), &need));
            count(ccmi_decode_batch_dev_rs_plan(sp.data(), ln.data(), n, nullptr, bd, chroma, &fmts[k], &rs, geom.data(),
                                                nullptr, &need));
        }
    count(ccmi_decode_batch_dev_rs_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &fmts[1], nullptr, geom.data(),
                                        info.data(), &need));
    {
        // the run entry point with capacities one byte short of what its own plan asks for the
        // output size: rejected before any GPU work
        ccmi_tensor_fmt f = fmts[0];
        f.colour = CCMI_COLOUR_RGB;
        const ccmi_resample rs{9, 5, CCMI_FILTER_TRIANGLE};
        std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
        std::vector<size_t> caps(n, 3 * 9 * 5 * 4 - 1);
        const int rc = ccmi_decode_batch_dev_rs(sp.data(), ln.data(), n, rects.data(), outs.data(), caps.data(), &f, &rs, bd,
                                                chroma, nullptr, 0, nullptr);
        if (rc == CCMI_OK) abort();
        count(rc);
        int batched = -1, per_frame = -1;
        if (ccmi_decode_last_tail_groups(&batched, &per_frame) != CCMI_OK || batched != 0 || per_frame != 0) abort();
    }
    {
        // the run entry point with capacities one byte short of what its own plan asks (or 0 when
        // the plan fails): rejected before any GPU work, the made-up pointers are never used
        ccmi_tensor_fmt f = fmts[1];
        f.colour = CCMI_COLOUR_RGB;
        std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
        std::vector<size_t> caps(n, 0);
        if (ccmi_decode_batch_dev_fmt_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &f, geom.data(), nullptr, &need) ==
            CCMI_OK)
            for (int i = 0; i < n; ++i)
                caps[i] = (2 * (size_t)f.stride_c + (size_t)(geom[i].height - 1) * f.stride_y +
                           (size_t)(geom[i].width - 1) * f.stride_x + 1) * 4 - 1;
        const int rc = ccmi_decode_batch_dev_fmt(sp.data(), ln.data(), n, rects.data(), outs.data(), caps.data(), &f, bd, chroma,
                                                 nullptr, 0, nullptr);
        if (rc == CCMI_OK) abort();
        count(rc);
    }
    // the warping sink: one matrix set per case, the same matrix for every frame
    const float inf = 1.f / 0.f, top = 4194304.f;
    const float mats[][6] = {{1, 0, 0, 0, 1, 0},          {1, 0, 3, 0, 1, 5},           {-1, 0, 64, 0, 1, 2},
                             {0.866f, -0.5f, 40, 0.5f, 0.866f, -20},                   {0.01f, 0, 7.5f, 0, 0.01f, 7.5f},
                             {1, 0, 1e6f, 0, 1, 1e6f},    {1, 0, -1e6f, 0, 1, -1e6f},   {0, 0, 5.25f, 0, 0, 9.75f},
                             {0, 0, 0, 0, 0, 0},          {1, 1, 0, 1, 1, 0},           {0, 0, top, 0, 0, -top},
                             {0, 0, 4194304.5f, 0, 1, 0}, {1, 0, 0, 300000, 0, 0},      {inf, 0, 0, 0, 1, 0},
                             {1, 0, 0, 0, 1, -inf},       {0.f / 0.f, 0, 0, 0, 1, 0},  {3e38f, 3e38f, 3e38f, 1, 1, 1}};
    const ccmi_warp sizes_wp[] = {{224, 224, CCMI_PAD_FILL, {0.5f, 0.5f, 0.5f}, nullptr}, {1, 1, CCMI_PAD_EDGE, {0, 0, 0}, nullptr},
                                  {16384, 3, CCMI_PAD_EDGE, {0, 0, 0}, nullptr},         {7, 16384, CCMI_PAD_FILL, {0, 1, 0}, nullptr},
                                  {0, 8, 0, {0, 0, 0}, nullptr},                         {8, 16385, 0, {0, 0, 0}, nullptr},
                                  {0x7fffffff, 0x7fffffff, 1, {0, 0, 0}, nullptr},       {8, 8, 2, {0, 0, 0}, nullptr},
                                  {8, 8, 0, {0, inf, 0}, nullptr},                       {8, 8, 1, {0.f / 0.f, 0, 0}, nullptr}};
    float *mat = static_cast<float *>(malloc(sizeof(float) * 6 * n));
    ccmi_rect *win = static_cast<ccmi_rect *>(malloc(sizeof(ccmi_rect) * n));
    for (const auto &m : mats) {
        for (int i = 0; i < n; ++i) memcpy(mat + 6 * i, m, sizeof m);
        for (ccmi_warp wp : sizes_wp) {
            wp.matrix = mat;
            for (size_t k = 1; k < fmts.size(); k += 6) {
                const int rc = ccmi_decode_batch_dev_warp_plan(sp.data(), ln.data(), n, bd, chroma, &fmts[k], &wp, geom.data(),
                                                               info.data(), win, &need);
                count(rc);
                if (rc == CCMI_OK) // the window is never empty and lies in the frame the header names
                    for (int i = 0; i < n; ++i)
                        if (win[i].w < 1 || win[i].h < 1 || win[i].x < 0 || win[i].y < 0 || geom[i].width != wp.out_w) abort();
                count(ccmi_decode_batch_dev_warp_plan(sp.data(), ln.data(), n, bd, chroma, &fmts[k], &wp, geom.data(), nullptr,
                                                      nullptr, &need));
            }
        }
    }
    {
        // NULL warp / matrix, and the run entry point with capacities one byte short: rejected
        // before any GPU work, the made-up pointers are never used
        ccmi_warp wp = sizes_wp[1];
        count(ccmi_decode_batch_dev_warp_plan(sp.data(), ln.data(), n, bd, chroma, &fmts[1], &wp, geom.data(), nullptr, win, &need));
        count(ccmi_decode_batch_dev_warp_plan(sp.data(), ln.data(), n, bd, chroma, &fmts[1], nullptr, geom.data(), nullptr, win,
                                              &need));
        memcpy(mat, mats[3], sizeof mats[3]);
        for (int i = 1; i < n; ++i) memcpy(mat + 6 * i, mats[1], sizeof mats[1]);
        wp = ccmi_warp{9, 5, CCMI_PAD_EDGE, {0, 0, 0}, mat};
        ccmi_tensor_fmt f = fmts[0];
        f.colour = CCMI_COLOUR_RGB;
        std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
        std::vector<size_t> caps(n, 3 * 9 * 5 * 4 - 1);
        const int rc = ccmi_decode_batch_dev_warp(sp.data(), ln.data(), n, outs.data(), caps.data(), &f, &wp, bd, chroma, nullptr,
                                                  0, nullptr);
        if (rc == CCMI_OK) abort();
        count(rc);
    }
    {
        // the colouring sink: the counts sit in a heap block of exactly n ints and the ops in one of
        // exactly their sum, so a read past either is reported.  Frame i of a case takes the case's
        // first (i % (len + 1)) ops; cases: every kind, 8 ops, 9 ops, an unknown op, two contrast ops,
        // a negative and two non-finite factors, a non-finite matrix entry; each with a region, with
        // a resample, with a warp, and with both (refused)
        const float nan = 0.f / 0.f;
        const ccmi_colour_op B{CCMI_COL_BRIGHTNESS, {1.25f}}, S{CCMI_COL_SATURATION, {0.5f}}, K{CCMI_COL_CONTRAST, {1.5f}},
            M{CCMI_COL_MATRIX, {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0}}, U{7, {1.f}}, N{CCMI_COL_BRIGHTNESS, {-0.5f}},
            I{CCMI_COL_SATURATION, {inf}}, Q{CCMI_COL_CONTRAST, {nan}}, X{CCMI_COL_MATRIX, {1, 0, 0, 0, 0, nan, 0, 0, 0, 0, 1, 0}};
        const std::vector<std::vector<ccmi_colour_op>> cases = {
            {B, S, K, M}, {M, M, M, M, K, S, B, B}, {B, B, B, B, B, B, B, B, B}, {B, U}, {K, B, K}, {S, N}, {I}, {M, Q}, {X}, {}};
        const ccmi_resample rs{9, 5, CCMI_FILTER_TRIANGLE};
        for (int i = 0; i < n; ++i) memcpy(mat + 6 * i, mats[3], sizeof mats[3]);
        ccmi_warp wp{9, 5, CCMI_PAD_FILL, {0.1f, 0.2f, 0.3f}, mat};
        for (const auto &cs : cases) {
            int *cnt = static_cast<int *>(malloc(sizeof(int) * n));
            size_t tot = 0;
            for (int i = 0; i < n; ++i) tot += (size_t)(cnt[i] = (int)((size_t)i % (cs.size() + 1)));
            if (n == 1) tot = (size_t)(cnt[0] = (int)cs.size());
            ccmi_colour_op *ops = static_cast<ccmi_colour_op *>(malloc(tot ? sizeof(ccmi_colour_op) * tot : 1));
            for (size_t k = 0, i = 0; (int)i < n; ++i)
                for (int e = 0; e < cnt[i]; ++e) ops[k++] = cs[(size_t)e];
            const ccmi_colour col{cnt, ops};
            const ccmi_tensor_fmt &f = fmts[1];
            count(ccmi_decode_batch_dev_col_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &f, nullptr, nullptr, &col,
                                                 geom.data(), info.data(), nullptr, &need));
            count(ccmi_decode_batch_dev_col_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &f, &rs, nullptr, &col,
                                                 geom.data(), nullptr, nullptr, &need));
            count(ccmi_decode_batch_dev_col_plan(sp.data(), ln.data(), n, nullptr, bd, chroma, &f, nullptr, &wp, &col, geom.data(),
                                                 info.data(), win, &need));
            int rc = ccmi_decode_batch_dev_col_plan(sp.data(), ln.data(), n, nullptr, bd, chroma, &f, &rs, &wp, &col, geom.data(),
                                                    nullptr, nullptr, &need);
            if (rc == CCMI_OK) abort();
            count(rc);
            // the run entry point with capacities one byte short: rejected before any GPU work
            std::vector<void *> outs(n, reinterpret_cast<void *>(uintptr_t(1) << 40));
            std::vector<size_t> caps(n, 3 * 9 * 5 * 4 - 1);
            ccmi_tensor_fmt g = fmts[0];
            g.colour = CCMI_COLOUR_RGB;
            rc = ccmi_decode_batch_dev_col(sp.data(), ln.data(), n, rects.data(), outs.data(), caps.data(), &g, &rs, nullptr, &col,
                                           bd, chroma, nullptr, 0, nullptr);
            if (rc == CCMI_OK) abort();
            count(rc);
            free(ops);
            free(cnt);
        }
        const ccmi_colour nocount{nullptr, nullptr};
        count(ccmi_decode_batch_dev_col_plan(sp.data(), ln.data(), n, rects.data(), bd, chroma, &fmts[1], nullptr, nullptr, &nocount,
                                             geom.data(), nullptr, nullptr, &need));
    }
    // the latent store: layout at every element type, a plan-only handle (no GPU call), and the
    // render planning over it: in order, through an index with repeats and out-of-range entries
    void *out0 = nullptr;
    size_t cap0 = 0;
    std::vector<size_t> each(n);
    size_t store = 0;
    for (int type = 0; type < 4; ++type)
        count(ccmi_latents_plan(sp.data(), ln.data(), n, type, &store, type & 1 ? each.data() : nullptr, &need));
    ccmi_latents *h = nullptr;
    count(ccmi_latents_decode(sp.data(), ln.data(), n, CCMI_LATENT_I16, nullptr, 0, nullptr, 0, nullptr, &h));
    if (!h) {
        free(mir);
        free(mat);
        free(win);
        return;
    }
    std::vector<int> idx(n + 2);
    std::vector<ccmi_rect> rr(n + 2);
    for (int j = 0; j < n + 2; ++j) idx[j] = (n - 1 - j % n + n) % n, rr[j] = rects[idx[j]];
    std::vector<ccmi_frame_geom> g2(n + 2);
    std::vector<ccmi_roi_info> i2(n + 2);
    for (int sample = 0; sample < 3; ++sample) {
        count(ccmi_latents_render_plan(h, nullptr, n, rects.data(), bd, chroma, sample, geom.data(), info.data(), &need));
        count(ccmi_latents_render_plan(h, nullptr, n, nullptr, bd, chroma, sample, geom.data(), nullptr, &need));
        count(ccmi_latents_render_plan(h, idx.data(), n + 2, rr.data(), bd, chroma, sample, g2.data(), i2.data(), &need));
    }
    idx[n] = n;
    count(ccmi_latents_render_plan(h, idx.data(), n + 2, nullptr, bd, chroma, 1, g2.data(), i2.data(), &need));
    idx[0] = -1;
    count(ccmi_latents_render_plan(h, idx.data(), n + 2, nullptr, bd, chroma, 1, g2.data(), i2.data(), &need));
    count(ccmi_latents_render_plan(h, nullptr, n + 1, nullptr, bd, chroma, 1, g2.data(), nullptr, &need));
    for (const ccmi_tensor_fmt &f : fmts) { // the mirror array has n entries: frames in order only
        count(ccmi_latents_render_fmt_plan(h, nullptr, n, rects.data(), bd, chroma, &f, geom.data(), info.data(), &need));
        count(ccmi_latents_render_fmt_plan(h, nullptr, n, nullptr, bd, chroma, &f, geom.data(), nullptr, &need));
    }
    count(ccmi_latents_render_fmt(h, nullptr, n, nullptr, &out0, &cap0, &fmts[1], bd, chroma, nullptr, 0, nullptr)); // plan-only
    for (const ccmi_resample &rs : sizes_rs) {
        count(ccmi_latents_render_rs_plan(h, nullptr, n, rects.data(), bd, chroma, &fmts[1], &rs, geom.data(), info.data(), &need));
        count(ccmi_latents_render_rs_plan(h, nullptr, n, nullptr, bd, chroma, &fmts[13], &rs, geom.data(), nullptr, &need));
    }
    count(ccmi_latents_render_rs_plan(h, nullptr, n, nullptr, bd, chroma, &fmts[1], nullptr, geom.data(), nullptr, &need));
    count(ccmi_latents_render_rs(h, nullptr, n, nullptr, &out0, &cap0, &fmts[1], &sizes_rs[0], bd, chroma, nullptr, 0,
                                 nullptr)); // plan-only
    for (const auto &m : mats) { // the matrix block has n entries: frames in order only
        for (int i = 0; i < n; ++i) memcpy(mat + 6 * i, m, sizeof m);
        for (ccmi_warp wp : sizes_wp) {
            wp.matrix = mat;
            count(ccmi_latents_render_warp_plan(h, nullptr, n, bd, chroma, &fmts[1], &wp, geom.data(), info.data(), win, &need));
            count(ccmi_latents_render_warp_plan(h, idx.data() + 1, n, bd, chroma, &fmts[13], &wp, geom.data(), nullptr, nullptr,
                                                &need));
        }
    }
    {
        ccmi_warp wp = sizes_wp[0];
        wp.matrix = mat;
        count(ccmi_latents_render_warp(h, nullptr, n, &out0, &cap0, &fmts[1], &wp, bd, chroma, nullptr, 0, nullptr)); // plan-only
    }
    void *out = nullptr;
    size_t cap = 0;
    count(ccmi_latents_render(h, nullptr, n, nullptr, &out, &cap, 1, bd, chroma, nullptr, 0, nullptr)); // plan-only: an error
    if (ccmi_latents_count(h) != n) abort();
    ccmi_latents_free(h);
    free(mir);
    free(mat);
    free(win);
}

std::vector<ccmi_rect> rects_of(int w, int h)
{
    const int a = w / 3 > 0 ? w / 3 : 1, b = h / 3 > 0 ? h / 3 : 1;
    return {{0, 0, w, h},         {0, 0, 1, 1},         {w - 1, 0, 1, 1},     {0, h - 1, 1, 1},     {w - 1, h - 1, 1, 1},
            {1, 1, w > 1 ? w - 1 : 1, h > 1 ? h - 1 : 1}, {0, b, a, b},       {a, 0, a, b},         {w - a, b, a, b},
            {a, h - b, a, b},     {-1, b, a, b},        {a, -1, a, b},        {w - a + 1, b, a, b}, {a, h - b + 1, a, b},
            {2, 2, 0, 4},         {2 * (w / 4), 2 * (h / 4), a, b},           {0x7fffffff, 0, 1, 1}, {0, 0, 0x7fffffff, 0x7fffffff}};
}

} // namespace

int main(int argc, char **argv)
{
    std::vector<Stream> all;
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
        all.push_back(exact_copy(buf.data(), buf.size()));
    }
    if (all.empty()) {
        fprintf(stderr, "usage: decode_plan_san stream.cool ...\n");
        return 2;
    }
    const int bds[] = {0, 8, 10, 16}, chromas[] = {0, 420, 444};
    for (size_t i = 0; i < all.size(); ++i) {
        const Stream &s = all[i];
        const int h = s.n >= 6 ? (s.p[2] << 8) | s.p[3] : 1, w = s.n >= 6 ? (s.p[4] << 8) | s.p[5] : 1;
        for (const ccmi_rect &r : rects_of(w, h))
            for (int bd : bds)
                for (int ch : chromas) plan_all({s}, {r}, bd, ch);
        const size_t hdr = s.n >= 11 ? 9 + (((size_t)s.p[9] << 8) | s.p[10]) : s.n;
        for (size_t cut = 0; cut <= s.n && cut <= hdr + 8; ++cut) {
            const Stream t = exact_copy(s.p, cut);
            plan_all({t}, {ccmi_rect{0, 0, w, h}}, 0, 0);
            plan_all({t}, {ccmi_rect{2, 2, w / 2 > 0 ? w / 2 : 1, h / 2 > 0 ? h / 2 : 1}}, 8, 420);
            free(t.p);
        }
    }
    for (size_t i = 0; i < all.size(); i += 7) {
        std::vector<Stream> b(all.begin() + i, all.begin() + std::min(all.size(), i + 7));
        std::vector<ccmi_rect> rects;
        for (size_t j = 0; j < b.size(); ++j) {
            const int h = (b[j].p[2] << 8) | b[j].p[3], w = (b[j].p[4] << 8) | b[j].p[5];
            rects.push_back(rects_of(w, h)[(i + j) % 10]);
        }
        for (int bd : bds)
            for (int ch : chromas) plan_all(b, rects, bd, ch);
    }
    {
        std::vector<ccmi_rect> rects;
        for (const Stream &s : all) rects.push_back(ccmi_rect{0, 0, (s.p[4] << 8) | s.p[5], (s.p[2] << 8) | s.p[3]});
        plan_all(all, rects, 0, 0);
    }
    for (Stream &s : all) free(s.p);
    printf("decode_plan_san: %ld calls, %ld succeeded\n", g_calls, g_ok);
    return g_ok > 0 ? 0 : 1;
}
