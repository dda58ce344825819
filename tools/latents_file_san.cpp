// latents_file_san.cpp -- stand-alone host program for a sanitizer run of the latent-file reader's
// host side (dec_store_file.cpp: ccmi_latents_file_head, ccmi_latents_import_plan, the plan-only
// ccmi_latents_import) on a machine without a GPU, the sibling of decode_plan_san.cpp.  The inputs
// are META blocks (HEAD | INDEX) named on the command line -- tests/golden/latent_meta/*.meta, the
// reference writer's META of the committed streams at I8 / I16 / I32 / SEG -- and, made from each:
// every truncation from 0 bytes to its length, and every single-byte replacement by 0x00, 0xFF and
// +1 within its first 4 KiB, once with index_sum left alone and once with it recomputed (so that
// the record parser, not the checksum, meets the damage).  Every input sits in a heap block of
// exactly its length, so a read past its end is reported.  Whatever handle an input yields goes
// through ccmi_latents_count / _stream_info, ccmi_latents_export_plan and the four render plans.
// No HIP call is made.
//
//   cd cool-chic_amd && hipcc -O1 -g -std=c++17 -fwrapv --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -x hip ../tools/latents_file_san.cpp csrc/dec_store_file.cpp csrc/dec_store.cpp csrc/dec_plan.cpp \
//       csrc/dec_host.cpp csrc/ccmi_api.cpp csrc/dec_arm.hip csrc/dec_tail.hip csrc/dec_out.hip \
//       csrc/dec_latents.hip -o /tmp/latents_file_san
//   /tmp/latents_file_san ../tests/golden/latent_meta/*.meta
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../cool-chic_amd/csrc/ccmi_internal.h"

// the float forward path is not linked: ccmi_api.cpp only needs the symbols
int ccmi_launch_arm_f32(const ccmi_arm_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_ups_f32(const ccmi_ups_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_syn_f32(const ccmi_syn_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }
int ccmi_launch_post_f32(const ccmi_post_args *, hipStream_t) { return CCMI_ERR_UNSUPPORTED; }

namespace {

long g_calls = 0, g_ok = 0, g_inputs = 0, g_handles = 0;

int count(int rc)
{
    ++g_calls;
    if (rc == CCMI_OK) ++g_ok;
    return rc;
}

// index_sum (bytes 40..55) recomputed over the bytes behind the head, as the contract states it
void fix_index_sum(std::vector<uint8_t> &m)
{
    if (m.size() < 64) return;
    uint64_t s0 = 0, s1 = 0;
    const size_t n = m.size() - 64;
    for (size_t i = 0; i < n; i += 4) {
        uint32_t w = 0;
        memcpy(&w, m.data() + 64 + i, std::min<size_t>(4, n - i));
        s0 += w;
        s1 += (uint64_t)(i / 4 + 1) * w;
    }
    memcpy(m.data() + 40, &s0, 8);
    memcpy(m.data() + 48, &s1, 8);
}

void plans_of(const ccmi_latents *h)
{
    const int n = ccmi_latents_count(h);
    for (int i = -1; i <= n; ++i) {
        int t = 0;
        size_t nb = 0;
        count(ccmi_latents_stream_info(h, i, &t, &nb));
    }
    size_t a = 0, b = 0, c = 0;
    count(ccmi_latents_export_plan(h, nullptr, n, &a, &b, &c));
    const int m = std::min(n, 4);
    std::vector<int> index(m);
    for (int j = 0; j < m; ++j) index[j] = n - 1 - j;
    std::vector<ccmi_rect> rects(m, ccmi_rect{2, 4, 66, 34});
    std::vector<ccmi_frame_geom> geom(m);
    std::vector<ccmi_roi_info> info(m);
    std::vector<ccmi_rect> window(m);
    count(ccmi_latents_export_plan(h, index.data(), m, &a, &b, &c));
    ccmi_tensor_fmt fmt{};
    fmt.elem = CCMI_ELEM_F32;
    fmt.colour = CCMI_COLOUR_RGB;
    for (int k = 0; k < 3; ++k) fmt.scale[k] = 1.f;
    const ccmi_resample rs{24, 16, CCMI_FILTER_TRIANGLE};
    std::vector<float> mat;
    for (int j = 0; j < m; ++j) {
        const float one[6] = {0.9f, -0.3f, 10.f, 0.3f, 0.9f, 6.f};
        mat.insert(mat.end(), one, one + 6);
    }
    ccmi_warp wp{};
    wp.out_w = 24, wp.out_h = 16, wp.pad = CCMI_PAD_FILL, wp.matrix = mat.data();
    size_t need = 0;
    for (const ccmi_rect *roi : {static_cast<const ccmi_rect *>(nullptr), static_cast<const ccmi_rect *>(rects.data())}) {
        for (int sample = 0; sample < 3; ++sample)
            count(ccmi_latents_render_plan(h, index.data(), m, roi, 0, 0, sample, geom.data(), info.data(), &need));
        count(ccmi_latents_render_fmt_plan(h, index.data(), m, roi, 0, 0, &fmt, geom.data(), info.data(), &need));
        count(ccmi_latents_render_rs_plan(h, index.data(), m, roi, 0, 0, &fmt, &rs, geom.data(), info.data(), &need));
    }
    count(ccmi_latents_render_warp_plan(h, index.data(), m, 0, 444, &fmt, &wp, geom.data(), info.data(), window.data(),
                                        &need));
}

// one input, in a heap block of exactly its length
void run(const uint8_t *src, size_t n)
{
    ++g_inputs;
    uint8_t *p = static_cast<uint8_t *>(malloc(n ? n : 1));
    if (n) memcpy(p, src, n);
    int ns = 0;
    size_t nmeta = 0, nfile = 0;
    if (n >= 64) count(ccmi_latents_file_head(p, 64, &ns, &nmeta, &nfile));
    count(ccmi_latents_file_head(p, n, &ns, &nmeta, &nfile));
    const int ranges[4][2] = {{0, -1}, {1, 1}, {0, 1}, {2, -1}};
    for (const auto &r : ranges) {
        size_t off = 0, bytes = 0, ws = 0, each[8] = {};
        // each[] holds 8: a count above it is not passed the array
        const int rc = count(ccmi_latents_import_plan(p, n, r[0], r[1], &off, &bytes, nullptr, &ws));
        if (rc == CCMI_OK && ns - r[0] <= 8) count(ccmi_latents_import_plan(p, n, r[0], r[1], &off, &bytes, each, &ws));
        ccmi_latents *h = nullptr;
        uint32_t flags[8] = {};
        const bool room = rc == CCMI_OK && ns - r[0] <= 8;
        if (count(ccmi_latents_import(p, n, r[0], r[1], nullptr, 0, nullptr, 0, nullptr, 0, nullptr, room ? flags : nullptr,
                                      &h)) == CCMI_OK) {
            ++g_handles;
            plans_of(h);
            ccmi_latents_free(h);
        } else if (h) {
            fprintf(stderr, "a refused import left a handle\n");
            exit(1);
        }
    }
    free(p);
}

} // namespace

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 1;
        }
        std::vector<uint8_t> meta;
        uint8_t buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) meta.insert(meta.end(), buf, buf + k);
        fclose(f);
        const long before = g_handles;
        run(meta.data(), meta.size());
        if (g_handles == before) {
            fprintf(stderr, "%s: the intact META was refused: %s\n", argv[a], ccmi_last_error());
            return 1;
        }
        for (size_t n = 0; n < meta.size(); ++n) run(meta.data(), n);
        const size_t lim = std::min<size_t>(meta.size(), 4096);
        for (size_t at = 0; at < lim; ++at)
            for (int kind = 0; kind < 3; ++kind)
                for (int fix = 0; fix < 2; ++fix) {
                    std::vector<uint8_t> m = meta;
                    m[at] = kind == 0 ? 0x00 : kind == 1 ? 0xFF : (uint8_t)(m[at] + 1);
                    if (fix) fix_index_sum(m);
                    run(m.data(), m.size());
                }
    }
    printf("%ld inputs, %ld calls, %ld returned CCMI_OK, %ld handles planned\n", g_inputs, g_calls, g_ok, g_handles);
    return 0;
}
