// decode_cubic_san.cpp -- stand-alone host program for a sanitizer run of the planner's bicubic
// paths (dec_plan.cpp: tensor_fmt, warp_check, warp_window) on a machine without a GPU, in the form
// of tools/decode_plan_san.cpp: every filter value of ccmi_resample around the accepted ones (0, 2,
// 0x102), every pad value of ccmi_warp around the accepted ones (0, 1, 0x100, 0x101, 0x300, 0x301),
// the cubic warp's windows at the frame's corners, across its edges, far outside it and under singular
// matrices (checked against the rule of ccmi.h, recomputed here, and against the bilinear window, which
// they must contain), and the extreme sizes (outputs of 1 and 16384, regions of 1 x 1 and the whole
// frame), through the decode and the latent-store entry points, with colour ops and through the run
// entry points with capacities they must reject.  The matrices sit in a heap block of exactly 6 n
// floats and the windows in one of exactly n rects.  No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_cubic_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_tone.hip \
//       csrc/dec_latents.hip -o /tmp/decode_cubic_san
//   /tmp/decode_cubic_san $(find ../tests/golden/cool ../tests/golden/cool_synth -name '*.cool')
#include <math.h>
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

long g_calls = 0, g_ok = 0;

int count(int rc)
{
    ++g_calls;
    if (rc == CCMI_OK) ++g_ok;
    return rc;
}

void must(bool ok, const char *what)
{
    if (ok) return;
    fprintf(stderr, "decode_cubic_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

bool filter_ok(int f) { return f == 0 || f == 2 || f == 0x102; }
bool pad_ok(int p) { return p == 0 || p == 1 || p == 0x100 || p == 0x101 || p == 0x300 || p == 0x301; }

// the window rule of ccmi.h for an h x w frame, reach 1 (bilinear) or 2 (cubic)
ccmi_rect window_rule(const float *m, int ow, int oh, int h, int w, bool even, int reach)
{
    const double cx[2] = {0.5, ow - 0.5}, cy[2] = {0.5, oh - 0.5};
    int lo[2], hi[2];
    for (int r = 0; r < 2; ++r) {
        double a = 0, b = 0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                const double v = (double)m[3 * r] * cx[i] + (double)m[3 * r + 1] * cy[j] + (double)m[3 * r + 2];
                if ((i | j) == 0 || v < a) a = v;
                if ((i | j) == 0 || v > b) b = v;
            }
        const double last = (r == 0 ? w : h) - 1;
        lo[r] = (int)std::min(std::max(floor(a - 0.5) - reach, 0.0), last);
        hi[r] = (int)std::min(std::max(floor(b - 0.5) + reach + 1, 0.0), last) + 1;
        if (even) lo[r] &= ~1, hi[r] = (hi[r] + 1) & ~1;
    }
    return ccmi_rect{lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]};
}

void run(const uint8_t *p, size_t len)
{
    const int h = (p[2] << 8) | p[3], w = (p[4] << 8) | p[5];
    const int n = 3;
    const uint8_t *sp[n] = {p, p, p};
    const size_t ln[n] = {len, len, len};
    ccmi_frame_geom geom[n];
    ccmi_roi_info info[n];
    size_t need = 0, need0 = 0;
    ccmi_tensor_fmt f{};
    f.elem = CCMI_ELEM_BF16, f.colour = CCMI_COLOUR_RGB;
    for (int c = 0; c < 3; ++c) f.scale[c] = 4.f + c, f.bias[c] = -1.f;
    ccmi_latents *hd = nullptr;
    must(count(ccmi_latents_decode(sp, ln, n, CCMI_LATENT_I16, nullptr, 0, nullptr, 0, nullptr, &hd)) == CCMI_OK && hd, "plan-only handle");
    void *outs[n] = {reinterpret_cast<void *>(uintptr_t(1) << 40), reinterpret_cast<void *>(uintptr_t(1) << 40),
                     reinterpret_cast<void *>(uintptr_t(1) << 40)};

    // ---- the resize: filter values, extreme sizes, regions at the corners; the cubic plan is the triangle plan
    const int filters[] = {0, 1, 2, 3, -1, 77, 0x100, 0x101, 0x102, 0x103, 0x200, 0x202, 0x302, 0x7fffffff, (int)0x80000000};
    const int sizes[][2] = {{224, 224}, {1, 1}, {16384, 1}, {1, 16384}, {16384, 16384}, {0, 8}, {8, 16385}, {w, h}};
    const int a = w / 2 > 0 ? w / 2 : 1, b = h / 2 > 0 ? h / 2 : 1;
    const ccmi_rect regions[][n] = {{{0, 0, w, h}, {0, 0, 1, 1}, {w - 1, h - 1, 1, 1}},
                                    {{0, 0, 2, 2}, {2 * ((w - 2) / 2), 2 * ((h - 2) / 2), 2, 2}, {0, 0, 2 * (a / 2 > 0 ? a / 2 : 1), 2 * (b / 2 > 0 ? b / 2 : 1)}}};
    for (const auto &rg : regions)
        for (const auto &sz : sizes)
            for (int chroma : {0, 444}) {
                const ccmi_resample tri{sz[0], sz[1], 0};
                const int rc0 = count(ccmi_decode_batch_dev_rs_plan(sp, ln, n, rg, 0, chroma, &f, &tri, geom, info, &need0));
                for (int filt : filters) {
                    const ccmi_resample rs{sz[0], sz[1], filt};
                    need = 0;
                    const int rc = count(ccmi_decode_batch_dev_rs_plan(sp, ln, n, rg, 0, chroma, &f, &rs, geom, info, &need));
                    if (!filter_ok(filt)) must(rc == CCMI_ERR_ARG && strstr(ccmi_last_error(), "filter"), "an unknown filter is refused");
                    else must(rc == rc0 && (rc != CCMI_OK || need == need0), "the cubic resize plan is the triangle plan");
                    const int rr = count(ccmi_latents_render_rs_plan(hd, nullptr, n, rg, 0, chroma, &f, &rs, geom, nullptr, &need));
                    must((rr == CCMI_OK) == (rc == CCMI_OK), "render and decode plans agree");
                    size_t caps[n] = {0, 0, 0}; // too small: rejected before any GPU work
                    must(count(ccmi_decode_batch_dev_rs(sp, ln, n, rg, outs, caps, &f, &rs, 0, chroma, nullptr, 0, nullptr)) != CCMI_OK,
                         "the run entry point refuses a capacity of 0");
                }
            }

    // ---- the warp: pad values, windows at the corners, across the edges and far outside, extreme sizes
    const float inf = 1.f / 0.f, top = 4194304.f;
    const float mats[][6] = {{1, 0, 0, 0, 1, 0},      {1, 0, -3, 0, 1, -2},      {1, 0, (float)w - 4, 0, 1, (float)h - 4},
                             {1, 0, (float)w, 0, 1, (float)h},                   {1, 0, -9, 0, 1, -9},
                             {-1, 0, 4, 0, -1, 4},    {0.866f, -0.5f, 0, 0.5f, 0.866f, 0},
                             {0.866f, -0.5f, (float)w, 0.5f, 0.866f, (float)h},  {0.01f, 0, 0.4f, 0, 0.01f, 0.4f},
                             {1, 0, 1e6f, 0, 1, 1e6f}, {1, 0, -1e6f, 0, 1, -1e6f}, {0, 0, 5.25f, 0, 0, 9.75f},
                             {0, 0, 0, 0, 0, 0},      {0, 0, top, 0, 0, -top},   {40, 0, 0, 0, 40, 0},
                             {0, 0, 4194304.5f, 0, 1, 0}, {inf, 0, 0, 0, 1, 0},  {0.f / 0.f, 0, 0, 0, 1, 0}};
    const int pads[] = {0, 1, 2, 3, -1, 77, 0x100, 0x101, 0x102, 0x200, 0x201, 0x300, 0x301, 0x302, 0x400, 0x401, 0x700, 0x7fffffff,
                        (int)0x80000000, (int)0x80000100};
    const int wsizes[][2] = {{224, 224}, {1, 1}, {16384, 1}, {1, 16384}, {9, 5}, {0, 8}, {8, 16385}};
    float *mat = static_cast<float *>(malloc(sizeof(float) * 6 * n));
    ccmi_rect *win = static_cast<ccmi_rect *>(malloc(sizeof(ccmi_rect) * n)), *win1 = static_cast<ccmi_rect *>(malloc(sizeof(ccmi_rect) * n));
    for (const auto &m : mats) {
        for (int i = 0; i < n; ++i) memcpy(mat + 6 * i, m, sizeof m);
        for (const auto &sz : wsizes)
            for (int chroma : {0, 444}) {
                ccmi_warp lin{sz[0], sz[1], CCMI_PAD_EDGE, {0.1f, 0.2f, 0.3f}, mat};
                const int rc1 = count(ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, chroma, &f, &lin, geom, info, win1, &need0));
                for (int pad : pads) {
                    ccmi_warp wp{sz[0], sz[1], pad, {0.1f, 0.2f, 0.3f}, mat};
                    const int rc = count(ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, chroma, &f, &wp, geom, info, win, &need));
                    if (!pad_ok(pad) && sz[0] >= 1 && sz[1] >= 1 && sz[0] <= 16384 && sz[1] <= 16384)
                        must(rc == CCMI_ERR_ARG && strstr(ccmi_last_error(), "pad"), "an unknown pad is refused");
                    if (!pad_ok(pad)) must(rc != CCMI_OK, "an unknown pad is refused");
                    else must((rc == CCMI_OK) == (rc1 == CCMI_OK), "the flags change no other check");
                    if (rc == CCMI_OK) {
                        const bool even = geom[0].chroma == 420;
                        const int reach = pad & CCMI_WARP_CUBIC ? 2 : 1;
                        for (int i = 0; i < n; ++i) {
                            const ccmi_rect want = window_rule(m, sz[0], sz[1], h, w, even, reach), &g = win[i], &l = win1[i];
                            must(g.x == want.x && g.y == want.y && g.w == want.w && g.h == want.h, "the window is the rule's");
                            must(g.w >= 1 && g.h >= 1 && g.x >= 0 && g.y >= 0 && g.x + g.w <= w && g.y + g.h <= h, "the window lies in the frame");
                            must(g.x <= l.x && g.y <= l.y && g.x + g.w >= l.x + l.w && g.y + g.h >= l.y + l.h,
                                 "the cubic window holds the bilinear one");
                        }
                    }
                    count(ccmi_latents_render_warp_plan(hd, nullptr, n, 0, chroma, &f, &wp, geom, nullptr, win, &need));
                    count(ccmi_latents_render_warp_plan(hd, nullptr, n, 0, chroma, &f, &wp, geom, info, nullptr, &need));
                    size_t caps[n] = {0, 0, 0};
                    must(count(ccmi_decode_batch_dev_warp(sp, ln, n, outs, caps, &f, &wp, 0, chroma, nullptr, 0, nullptr)) != CCMI_OK,
                         "the run entry point refuses a capacity of 0");
                }
            }
    }

    // ---- with colour ops (the colour plan takes either geometry): cubic, clamped, refused together
    {
        int cnt[n] = {2, 0, 1};
        const ccmi_colour_op ops[3] = {{CCMI_COL_BRIGHTNESS, {1.25f}}, {CCMI_COL_CONTRAST, {1.5f}}, {CCMI_COL_SATURATION, {0.5f}}};
        const ccmi_colour col{cnt, ops};
        memcpy(mat, mats[6], sizeof mats[6]), memcpy(mat + 6, mats[7], sizeof mats[7]), memcpy(mat + 12, mats[3], sizeof mats[3]);
        const ccmi_resample rs{9, 5, CCMI_FILTER_CUBIC | CCMI_FILTER_CLAMP};
        const ccmi_warp wp{9, 5, CCMI_PAD_FILL | CCMI_WARP_CUBIC | CCMI_WARP_CLAMP, {0.1f, 0.2f, 0.3f}, mat};
        must(count(ccmi_decode_batch_dev_col_plan(sp, ln, n, regions[1], 0, 0, &f, &rs, nullptr, &col, geom, info, nullptr, &need)) == CCMI_OK,
             "colour ops after a cubic resize");
        must(count(ccmi_decode_batch_dev_col_plan(sp, ln, n, nullptr, 0, 444, &f, nullptr, &wp, &col, geom, info, win, &need)) == CCMI_OK,
             "colour ops after a cubic warp");
        must(count(ccmi_decode_batch_dev_col_plan(sp, ln, n, nullptr, 0, 444, &f, &rs, &wp, &col, geom, nullptr, nullptr, &need)) != CCMI_OK,
             "a resample and a warp together are refused");
    }
    ccmi_latents_free(hd);
    free(mat);
    free(win);
    free(win1);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: decode_cubic_san stream.cool ...\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        FILE *fp = fopen(argv[i], "rb");
        if (!fp) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::vector<uint8_t> buf;
        uint8_t tmp[4096];
        for (size_t k; (k = fread(tmp, 1, sizeof tmp, fp)) > 0;) buf.insert(buf.end(), tmp, tmp + k);
        fclose(fp);
        uint8_t *p = static_cast<uint8_t *>(malloc(buf.size() ? buf.size() : 1)); // exactly its length: a read past the end is reported
        memcpy(p, buf.data(), buf.size());
        if (buf.size() >= 6) run(p, buf.size());
        free(p);
    }
    printf("decode_cubic_san: %ld calls, %ld succeeded\n", g_calls, g_ok);
    return g_ok > 0 ? 0 : 1;
}
