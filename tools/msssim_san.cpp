// msssim_san.cpp -- stand-alone host program for a sanitizer run of the MS-SSIM stage's host checks
// (ccmi_msssim_workspace_bytes and the argument checks of ccmi_msssim_f32, dist_msssim.hip) on a
// machine without a GPU, in the form of decode_mix_san.cpp.  Every ccmi_msssim_args is a heap block
// of exactly its size; x, y, out, grad and the workspace are addresses that are never dereferenced
// (every call below is refused before any HIP call, or only sizes a workspace).  The workspace is
// checked against the formula of ccmi.h for every shape from 11 x 11 to 300 x 450, 1 to 5 scales,
// batches of 1, 7 and 960, with and without a gradient.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/msssim_san.cpp csrc/dist_msssim.hip csrc/ccmi_api.cpp -o /tmp/msssim_san
//   /tmp/msssim_san
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cool-chic_amd/csrc/ccmi_internal.h"

// the float forward path is not linked: ccmi_api.cpp only needs the symbols
int ccmi_launch_arm_f32(const ccmi_arm_args *, hipStream_t, int) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_ups_f32(const ccmi_ups_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_syn_f32(const ccmi_syn_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_post_f32(const ccmi_post_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }

namespace {

long g_calls = 0, g_refused = 0;

void fail(const char *what)
{
    fprintf(stderr, "msssim_san: %s (%s)\n", what, ccmi_last_error());
    abort();
}

ccmi_msssim_args *make(int h, int w, int S, int B, bool grad)
{
    ccmi_msssim_args *a = static_cast<ccmi_msssim_args *>(calloc(1, sizeof(ccmi_msssim_args)));
    a->batch = B, a->n_planes = 3, a->n_scales = S, a->clamp = 1;
    int64_t o = 0;
    for (int p = 0; p < 3; ++p) {
        const int hh = p ? h / 2 : h, ww = p ? w / 2 : w; // 4:2:0, packed
        a->h[p] = hh, a->w[p] = ww, a->x_off[p] = o, a->x_pitch[p] = ww, a->x_sub[p] = 1;
        o += (int64_t)hh * ww;
        a->channel_weights[p] = 1.f / 3;
    }
    float *fake = reinterpret_cast<float *>(0x1000);
    a->x = a->y = fake, a->x_stride = a->y_stride = o;
    for (int s = 0; s < S; ++s) a->weights[s] = 1.f / S;
    a->alpha_mse = 0.3f, a->beta_ms = 0.7f;
    a->out = fake, a->grad = grad ? fake : nullptr;
    a->workspace = fake, a->workspace_bytes = 0; // short: the run entry point is refused after every other check
    return a;
}

size_t al(size_t n) { return (4 * n + 255) / 256 * 256; }

size_t formula(const ccmi_msssim_args *a)
{
    size_t pyr = 0, pos = 0, tiles = 0;
    for (int p = 0; p < a->n_planes; ++p) {
        int h = a->h[p], w = a->w[p];
        for (int s = 0; s < a->n_scales; ++s) {
            if (h < 11 || w < 11) return 0;
            if (s) pyr += (size_t)h * w;
            pos += (size_t)(h - 10) * (w - 10);
            tiles += (size_t)((h - 10 + 21) / 22) * ((w - 10 + 31) / 32);
            h = (h + 1) / 2, w = (w + 1) / 2;
        }
    }
    const size_t B = (size_t)a->batch;
    return 2 * al(B * pyr) + al(2 * B * tiles) + al(16 * B) + (a->grad ? al(B * pyr) + al(3 * B * pos) : 0);
}

void refused(ccmi_msssim_args *a, const char *word)
{
    ++g_calls;
    if (ccmi_msssim_f32(a, nullptr) != CCMI_ERR_ARG || !strstr(ccmi_last_error(), word)) fail(word);
    ++g_refused;
    free(a);
}

} // namespace

int main()
{
    for (int h = 22; h <= 300; h += 7)
        for (int w = 22; w <= 450; w += 13)
            for (int S = 1; S <= 5; ++S)
                for (int B : {1, 7, 960})
                    for (int grad = 0; grad < 2; ++grad) {
                        ccmi_msssim_args *a = make(h, w, S, B, grad != 0);
                        ++g_calls;
                        const size_t want = formula(a);
                        if (ccmi_msssim_workspace_bytes(a) != want) fail("workspace formula");
                        // a valid shape is refused for its short workspace alone, an invalid one names plane and scale
                        refused(a, want ? "workspace" : "plane");
                    }
    ccmi_msssim_args *a;
    a = make(41, 43, 1, 2, true), a->out = nullptr, refused(a, "out is null");
    a = make(41, 43, 1, 2, true), a->x = nullptr, refused(a, "null");
    a = make(41, 43, 1, 2, true), a->x_sub[2] = 3, refused(a, "x_sub[2]");
    a = make(41, 43, 1, 2, true), a->x_sub[0] = 0, refused(a, "x_sub[0]");
    a = make(41, 43, 1, 2, true), a->weights[0] = -1.f, refused(a, "weights[0]");
    a = make(41, 43, 1, 2, true), a->weights[0] = NAN, refused(a, "weights[0]");
    a = make(41, 43, 1, 2, true), a->channel_weights[1] = INFINITY, refused(a, "channel_weights[1]");
    a = make(41, 43, 1, 2, true), a->alpha_mse = NAN, refused(a, "alpha_mse");
    a = make(41, 43, 1, 2, true), a->n_scales = 6, refused(a, "n_scales");
    a = make(41, 43, 1, 2, true), a->n_planes = 0, refused(a, "n_planes");
    a = make(41, 43, 1, 2, true), a->batch = 0, refused(a, "batch");
    a = make(41, 43, 1, 2, true), a->y_stride = 1, refused(a, "y_stride");
    a = make(41, 43, 1, 2, true), a->x_pitch[0] = 42, refused(a, "x_pitch");
    ++g_calls;
    if (ccmi_msssim_f32(nullptr, nullptr) != CCMI_ERR_ARG || ccmi_msssim_workspace_bytes(nullptr) != 0) fail("null args");
    printf("msssim_san: %ld calls, %ld refused as expected, no HIP call\n", g_calls, g_refused);
    return 0;
}
