// decode_persp_san.cpp -- stand-alone host program for a sanitizer run of the planner's projective
// paths (dec_plan.cpp: warp_check, warp_window, tensor_fmt with CCMI_WARP_PROJECTIVE) on a machine
// without a GPU, in the form of tools/decode_cubic_san.cpp: every pad value of ccmi_warp around the
// accepted ones (the affine six and 0x800, 0x801, 0x900, 0x901, 0xB00, 0xB01), the bounds of step 3a'
// in ccmi.h on both sides (S_r <= 2^22, D' > 0, S_r / D' <= 2^22, E_r <= 7/8: the decision recomputed
// here), denominators that vanish inside and outside the output grid, singular matrices, non-finite
// entries in each of the nine places, the extreme output sizes, and the window rule (the quotients at
// the four corner pixel centres, recomputed here), through the decode and the latent-store entry points,
// the _col / _flt / _tone plans and the run entry points with capacities they must reject.  The
// matrices sit in a heap block of exactly 9 n floats and the windows in one of exactly n rects, so a
// read with the wrong stride is reported.  No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/decode_persp_san.cpp csrc/dec_plan.cpp csrc/dec_host.cpp csrc/ccmi_api.cpp \
//       csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip csrc/dec_filter.hip csrc/dec_tone.hip \
//       csrc/dec_latents.hip -o /tmp/decode_persp_san
//   /tmp/decode_persp_san $(find ../tests/golden/cool ../tests/golden/cool_synth -name '*.cool')
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
    fprintf(stderr, "decode_persp_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

bool pad_ok(int p)
{
    const int base = p & ~CCMI_WARP_PROJECTIVE;
    return p >= 0 && (base == 0 || base == 1 || base == 0x100 || base == 0x101 || base == 0x300 || base == 0x301);
}

// the checks of step 3a' for an h x w frame: NULL if the matrix is accepted, else a word of the message
const char *refusal(const float *m, int ow, int oh, int h, int w)
{
    for (int k = 0; k < 9; ++k)
        if (!isfinite(m[k])) return "finite";
    const double eps = ldexp(1.0, -24), top = ldexp(1.0, 22);
    double S[3];
    for (int r = 0; r < 3; ++r) {
        S[r] = fabs((double)m[3 * r]) * ow + fabs((double)m[3 * r + 1]) * oh + fabs((double)m[3 * r + 2]);
        if (S[r] > top) return "2^22";
    }
    double D = 0;
    for (int c = 0; c < 4; ++c) {
        const double v = (double)m[6] * (c & 1 ? ow - 0.5 : 0.5) + (double)m[7] * (c & 2 ? oh - 0.5 : 0.5) + (double)m[8];
        if (c == 0 || v < D) D = v;
    }
    const double Dp = D - 3 * eps * S[2];
    if (!(Dp > 0)) return "denominator";
    if (S[0] / Dp > top || S[1] / Dp > top) return "2^22";
    for (int r = 0; r < 2; ++r) {
        const double L = (r == 0 ? w : h) + 3.0;
        if (3 * eps * (S[r] + L * S[2]) / Dp + 2 * eps * L > 0.875) return "too strong";
    }
    return nullptr;
}

// the window rule of ccmi.h for an h x w frame, reach 1 (bilinear) or 2 (cubic), on the quotients
ccmi_rect window_rule(const float *m, int ow, int oh, int h, int w, bool even, int reach)
{
    const double cx[2] = {0.5, ow - 0.5}, cy[2] = {0.5, oh - 0.5};
    int lo[2], hi[2];
    for (int r = 0; r < 2; ++r) {
        double a = 0, b = 0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                const double v = ((double)m[3 * r] * cx[i] + (double)m[3 * r + 1] * cy[j] + (double)m[3 * r + 2]) /
                                 ((double)m[6] * cx[i] + (double)m[7] * cy[j] + (double)m[8]);
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
    size_t need = 0, need6 = 0;
    ccmi_tensor_fmt f{};
    f.elem = CCMI_ELEM_BF16, f.colour = CCMI_COLOUR_RGB;
    for (int c = 0; c < 3; ++c) f.scale[c] = 4.f + c, f.bias[c] = -1.f;
    ccmi_latents *hd = nullptr;
    must(count(ccmi_latents_decode(sp, ln, n, CCMI_LATENT_I16, nullptr, 0, nullptr, 0, nullptr, &hd)) == CCMI_OK && hd, "plan-only handle");
    void *outs[n] = {reinterpret_cast<void *>(uintptr_t(1) << 40), reinterpret_cast<void *>(uintptr_t(1) << 40),
                     reinterpret_cast<void *>(uintptr_t(1) << 40)};

    const float inf = 1.f / 0.f, nan = 0.f / 0.f, top = 4194304.f, over = nextafterf(top, inf);
    const float W = (float)w, H = (float)h;
    const float mats[][9] = {
        {1, 0, 0, 0, 1, 0, 0, 0, 1},                        // the identity
        {1, 0, -3, 0, 1, -2, 0, 0, 1},                      // affine rows 0 0 1: the 6-entry call's plan
        {0.866f, -0.5f, W, 0.5f, 0.866f, H, 0, 0, 1},
        {-1, 0, 4, 0, -1, 4, 0, 0, 1},
        {1, 0, 1e6f, 0, 1, 1e6f, 0, 0, 1},                  // far outside
        {2, 0, 100, 0, 2, 50, 0.125f, 0, 1},                // a mild perspective
        {1, 0, 0, 0, 1, 0, 0.001f, 0.002f, 1},
        {37, 0, 74, 0, 37, 37, 0.037f, -0.0037f, 37},       // a common factor the quotient cancels
        {1, 0, 0, 0, 1, 0, -0.01f, -0.01f, 1},              // the denominator falls towards the far corner ...
        {1, 0, 0, 0, 1, 0, -1, 0, 4},                       // ... and vanishes inside an 8-wide grid
        {1, 0, 0, 0, 1, 0, -1, 0, 7.5f},                    // at the last pixel centre of an 8-wide output
        {1, 0, 0, 0, 1, 0, -1, 0, 7.5005f},                 // positive but too strong
        {1, 0, 0, 0, 1, 0, -1, 0, 7.6f},                    // vanishes just outside an 8-wide grid
        {1, 0, 0, 0, 1, 0, -1, 0, 300},                     // vanishes outside every small grid, inside a 16384-wide one
        {1, 0, 0, 0, 1, 0, 1, 1, -1},                       // negative at the first corner only (of small grids)
        {1, 0, 0, 0, 1, 0, 0, 0, 0},                        // no denominator
        {1, 0, 0, 0, 1, 0, 0, 0, -1},                       // negative everywhere
        {0, 0, 0, 0, 0, 0, 0, 0, 0},                        // singular
        {0, 0, 5.25f, 0, 0, 9.75f, 0, 0, 1},
        {0, 0, 7, 0, 0, 9, 0.5f, 0.5f, 1},                  // constant numerators
        {1, 2, 3, 2, 4, 6, 0, 0, 1},                        // rank 1
        {0, 0, top, 0, 0, -top, 0, 0, 2},                   // the reach bound, at it ...
        {0, 0, over, 0, 1, 0, 0, 0, 2},                     // ... and one float32 step above, per row
        {1, 0, 0, 0, 0, -over, 0, 0, 2},
        {1, 0, 0, 0, 1, 0, 0, 0, top},
        {1, 0, 0, 0, 1, 0, 0, 0, over},
        {0, 0, top, 0, 1, 0, 0, 0, 1},                      // S_0 / D' just above 2^22
        {0, 0, top, 0, 1, 0, 0, 0, 1.000001f},
        {1e30f, 0, 0, 0, 1, 0, 0, 0, 1e30f},
        {1, 0, 0, 0, 1, 0, 0, 0, 1e-30f},
    };
    const int pads[] = {0, 1, 2, -1, 77, 0x100, 0x101, 0x200, 0x300, 0x301, 0x400, 0x401, 0x700, 0x800, 0x801, 0x802, 0x880,
                        0x900, 0x901, 0xA00, 0xA01, 0xB00, 0xB01, 0xB02, 0xC00, 0xF01, 0x1000, 0x1800, 0x7fffffff, (int)0x80000000,
                        (int)0x80000800};
    const int wsizes[][2] = {{8, 8}, {224, 224}, {1, 1}, {16384, 1}, {1, 16384}, {9, 5}, {0, 8}, {8, 16385}};
    float *mat = static_cast<float *>(malloc(sizeof(float) * 9 * n)), *mat6 = static_cast<float *>(malloc(sizeof(float) * 6 * n));
    ccmi_rect *win = static_cast<ccmi_rect *>(malloc(sizeof(ccmi_rect) * n)), *win6 = static_cast<ccmi_rect *>(malloc(sizeof(ccmi_rect) * n));
    for (const auto &m : mats) {
        // frames 0 and 2 take the matrix, frame 1 the identity: a refusal names frame 0
        for (int i = 0; i < n; ++i) memcpy(mat + 9 * i, i == 1 ? mats[0] : m, sizeof m);
        const bool affine = m[6] == 0 && m[7] == 0 && m[8] == 1;
        for (int i = 0; i < n; ++i) memcpy(mat6 + 6 * i, i == 1 ? mats[0] : m, 6 * sizeof(float));
        for (const auto &sz : wsizes) {
            const bool size_ok = sz[0] >= 1 && sz[1] >= 1 && sz[0] <= 16384 && sz[1] <= 16384;
            for (int chroma : {0, 444})
                for (int pad : pads) {
                    ccmi_warp wp{sz[0], sz[1], pad, {0.1f, 0.2f, 0.3f}, pad >= 0 && (pad & CCMI_WARP_PROJECTIVE) ? mat : mat6};
                    need = 0;
                    const int rc = count(ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, chroma, &f, &wp, geom, info, win, &need));
                    if (!pad_ok(pad)) {
                        must(rc != CCMI_OK, "an unknown pad is refused");
                        if (size_ok) must(rc == CCMI_ERR_ARG && strstr(ccmi_last_error(), "pad"), "an unknown pad is named");
                    } else if ((pad & CCMI_WARP_PROJECTIVE) && size_ok) {
                        const char *why = refusal(m, sz[0], sz[1], h, w);
                        const bool odd420 = chroma == 0 && rc != CCMI_OK && strstr(ccmi_last_error(), "even");
                        if (why) must(rc == CCMI_ERR_ARG && strstr(ccmi_last_error(), why) && strstr(ccmi_last_error(), "frame 0") && need == 0,
                                      "the plan refuses what the rule refuses, naming the frame");
                        else must(rc == CCMI_OK || odd420, "the plan accepts what the rule accepts");
                        if (rc == CCMI_OK) {
                            const bool even = geom[0].chroma == 420;
                            const int reach = pad & CCMI_WARP_CUBIC ? 2 : 1;
                            for (int i = 0; i < n; ++i) {
                                const ccmi_rect want = window_rule(mat + 9 * i, sz[0], sz[1], h, w, even, reach), &g = win[i];
                                must(g.x == want.x && g.y == want.y && g.w == want.w && g.h == want.h, "the window is the rule's");
                                must(g.w >= 1 && g.h >= 1 && g.x >= 0 && g.y >= 0 && g.x + g.w <= w && g.y + g.h <= h, "the window lies in the frame");
                            }
                            if (affine) { // rows 0 0 1: the window and the geometry of the 6-entry call
                                ccmi_warp w6{sz[0], sz[1], pad & ~CCMI_WARP_PROJECTIVE, {0.1f, 0.2f, 0.3f}, mat6};
                                ccmi_frame_geom g6[n];
                                must(count(ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, chroma, &f, &w6, g6, nullptr, win6, &need6)) == CCMI_OK,
                                     "the 6-entry call of an accepted 0 0 1 matrix");
                                must(memcmp(win, win6, sizeof(ccmi_rect) * n) == 0 && need >= need6 && need - need6 <= 256,
                                     "a 0 0 1 matrix plans as its 6-entry call");
                                for (int i = 0; i < n; ++i)
                                    must(g6[i].width == geom[i].width && g6[i].height == geom[i].height && g6[i].elems == geom[i].elems, "geometry");
                            }
                        }
                    }
                    // every other plan that carries a warp decides alike
                    size_t nd = 0;
                    const int rl = count(ccmi_latents_render_warp_plan(hd, nullptr, n, 0, chroma, &f, &wp, geom, nullptr, win, &nd));
                    const int rcol = count(ccmi_decode_batch_dev_col_plan(sp, ln, n, nullptr, 0, chroma, &f, nullptr, &wp, nullptr, geom, info, win, &nd));
                    const int rflt = count(ccmi_decode_batch_dev_flt_plan(sp, ln, n, nullptr, 0, chroma, &f, nullptr, &wp, nullptr, nullptr, geom, info, nullptr, &nd));
                    const int rtone = count(ccmi_latents_render_tone_plan(hd, nullptr, n, nullptr, 0, chroma, &f, nullptr, &wp, nullptr, nullptr, nullptr, geom, nullptr, win, &nd));
                    must((rl == CCMI_OK) == (rc == CCMI_OK) && (rcol == CCMI_OK) == (rc == CCMI_OK) && (rflt == CCMI_OK) == (rc == CCMI_OK) &&
                             (rtone == CCMI_OK) == (rc == CCMI_OK),
                         "the render, colour, filter and tone plans agree with the warp plan");
                    size_t caps[n] = {0, 0, 0}; // too small: rejected before any GPU work
                    must(count(ccmi_decode_batch_dev_warp(sp, ln, n, outs, caps, &f, &wp, 0, chroma, nullptr, 0, nullptr)) != CCMI_OK,
                         "the run entry point refuses a capacity of 0");
                }
        }
    }

    // ---- a non-finite value in each of the nine places of the LAST frame: the last float of the block is read, none past it
    for (int k = 0; k < 9; ++k)
        for (float bad : {inf, -inf, nan}) {
            for (int i = 0; i < n; ++i) memcpy(mat + 9 * i, mats[5], sizeof mats[5]);
            mat[9 * (n - 1) + k] = bad;
            ccmi_warp wp{8, 8, CCMI_PAD_EDGE | CCMI_WARP_PROJECTIVE | CCMI_WARP_CUBIC, {0.1f, 0.2f, 0.3f}, mat};
            must(count(ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, 444, &f, &wp, geom, info, win, &need)) == CCMI_ERR_ARG &&
                     strstr(ccmi_last_error(), "finite") && strstr(ccmi_last_error(), "frame 2"),
                 "a non-finite entry of the last frame is named");
        }

    // ---- with colour ops, a filter and tone ops on a projective warp
    {
        int cnt[n] = {2, 0, 1};
        const ccmi_colour_op ops[3] = {{CCMI_COL_BRIGHTNESS, {1.25f}}, {CCMI_COL_CONTRAST, {1.5f}}, {CCMI_COL_SATURATION, {0.5f}}};
        const ccmi_colour col{cnt, ops};
        memcpy(mat, mats[5], sizeof mats[5]), memcpy(mat + 9, mats[6], sizeof mats[6]), memcpy(mat + 18, mats[7], sizeof mats[7]);
        const ccmi_warp wp{9, 5, CCMI_PAD_FILL | CCMI_WARP_CUBIC | CCMI_WARP_CLAMP | CCMI_WARP_PROJECTIVE, {0.1f, 0.2f, 0.3f}, mat};
        const ccmi_resample rs{9, 5, CCMI_FILTER_CUBIC};
        must(count(ccmi_decode_batch_dev_col_plan(sp, ln, n, nullptr, 0, 444, &f, nullptr, &wp, &col, geom, info, win, &need)) == CCMI_OK,
             "colour ops after a projective warp");
        must(count(ccmi_latents_render_col_plan(hd, nullptr, n, nullptr, 0, 444, &f, nullptr, &wp, &col, geom, info, win, &need)) == CCMI_OK,
             "colour ops after a projective warp, from the store");
        must(count(ccmi_decode_batch_dev_col_plan(sp, ln, n, nullptr, 0, 444, &f, &rs, &wp, &col, geom, nullptr, nullptr, &need)) != CCMI_OK,
             "a resample and a warp together are refused");
    }
    ccmi_latents_free(hd);
    free(mat);
    free(mat6);
    free(win);
    free(win6);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: decode_persp_san stream.cool ...\n");
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
    printf("decode_persp_san: %ld calls, %ld succeeded\n", g_calls, g_ok);
    return g_ok > 0 ? 0 : 1;
}
