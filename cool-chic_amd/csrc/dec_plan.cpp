// dec_plan.cpp -- path B: the header pass of a decode call (decode_plan): per-stream
// validation, output formats, region windows and the layout of the one device workspace.
// Host arithmetic only: no HIP runtime call in this file.
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>

#include "dec_plan.h"

namespace ccmi {

int out_format(const FrameHost &f, int out_bitdepth, int out_chroma, int as_yuv, OutFmt &o)
{
    o.bitdepth = out_bitdepth ? out_bitdepth : f.bitdepth;
    const int chroma = out_chroma ? out_chroma : (f.frame_data_type == 1 ? 420 : 444);
    const size_t bps = o.bitdepth <= 8 ? 1 : 2;
    const size_t npx = (size_t)f.h * f.w;
    o.header = 0;
    if (as_yuv) {
        if (o.bitdepth != 8 && o.bitdepth != 10)
            return ccmi_set_error(CCMI_ERR_UNSUPPORTED, "YUV output bitdepth must be 8 or 10 (got %d)", o.bitdepth);
        o.kind = chroma == 420 ? kYuv420 : kYuv444;
        o.payload = bps * (o.kind == kYuv420 ? npx + 2 * (size_t)(f.h / 2) * (f.w / 2) : 3 * npx);
    } else {
        if (o.bitdepth < 1 || o.bitdepth > 16) return ccmi_set_error(CCMI_ERR_ARG, "PPM bitdepth %d", o.bitdepth);
        o.kind = kPpm;
        o.header = (size_t)snprintf(o.hdr, sizeof o.hdr, "P6\n%d %d\n%d\n", f.w, f.h, (1 << o.bitdepth) - 1);
        o.payload = bps * 3 * npx;
    }
    return CCMI_OK;
}

namespace {

size_t sample_bytes(int sample) { return sample == CCMI_SAMPLE_U8 ? 1 : sample == CCMI_SAMPLE_U16 ? 2 : 4; }

// output of a device sink: planar 420 / 444 samples, no header; payload = bytes at the caller's pointer
int tensor_format(const FrameHost &f, int out_bitdepth, int out_chroma, int sample, OutFmt &o, size_t *elems,
                  const DecWindow &rect)
{
    if (sample != CCMI_SAMPLE_U8 && sample != CCMI_SAMPLE_U16 && sample != CCMI_SAMPLE_F32)
        return ccmi_set_error(CCMI_ERR_ARG, "decode: unknown sample type %d", sample);
    if (out_chroma != 0 && out_chroma != 420 && out_chroma != 444)
        return ccmi_set_error(CCMI_ERR_ARG, "decode: output chroma format %d (0, 420 or 444)", out_chroma);
    o.bitdepth = out_bitdepth ? out_bitdepth : f.bitdepth;
    if (o.bitdepth < 1 || o.bitdepth > 16) return ccmi_set_error(CCMI_ERR_ARG, "decode: output bitdepth %d", o.bitdepth);
    if (sample == CCMI_SAMPLE_U8 && o.bitdepth > 8)
        return ccmi_set_error(CCMI_ERR_ARG, "decode: %d-bit samples do not fit CCMI_SAMPLE_U8", o.bitdepth);
    const int chroma = out_chroma ? out_chroma : (f.frame_data_type == 1 ? 420 : 444);
    const size_t npx = (size_t)rect.h() * rect.w();
    o.kind = chroma == 420 ? kYuv420 : kYuv444;
    o.header = 0;
    *elems = o.kind == kYuv420 ? npx + 2 * (size_t)(rect.h() / 2) * (rect.w() / 2) : 3 * npx;
    o.payload = sample_bytes(sample) * *elems;
    return CCMI_OK;
}

size_t elem_bytes(int elem) { return elem == CCMI_ELEM_F32 ? 4 : 2; }

// region and output extents of a resample: the triangle's integer weights and their sums fit int32,
// the cubic's terms stay below 2^51 and their sums below 2^61 (int64)
constexpr int kMaxResample = 16384;

constexpr double kMaxWarpReach = 4194304.0; // 2^22: the bound on a warp's float32 positions

// A warp (ccmi_warp) of frame i: the checks that need no header.  After them every position of
// the output grid is finite and within 2^22 of the origin, so the window below is plain arithmetic.
// With CCMI_WARP_PROJECTIVE the matrix is 3 x 3 and the checks are those of step 3a' in ccmi.h, in
// double from the float32 entries, on the fh x fw frame: after them the float32 denominator is
// positive at every pixel, every quotient within 2^22 of the origin and within 7/8 pixel of the
// exact position wherever it lies within two taps of the frame.
int warp_check(const ccmi_warp &wp, int i, int fh, int fw)
{
    if (wp.out_w < 1 || wp.out_w > kMaxResample || wp.out_h < 1 || wp.out_h > kMaxResample)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: output size w %d h %d (1 .. %d)", i, wp.out_w, wp.out_h,
                              kMaxResample);
    // none, CCMI_WARP_CUBIC, or CCMI_WARP_CUBIC | CCMI_WARP_CLAMP, each with or without CCMI_WARP_PROJECTIVE
    const int flags = wp.pad & ~(1 | CCMI_WARP_PROJECTIVE);
    if (wp.pad < 0 || (flags != 0 && flags != CCMI_WARP_CUBIC && flags != (CCMI_WARP_CUBIC | CCMI_WARP_CLAMP)))
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: unknown pad %d", i, wp.pad);
    const bool persp = (wp.pad & CCMI_WARP_PROJECTIVE) != 0;
    const int entries = persp ? 9 : 6;
    const float *m = wp.matrix + entries * (size_t)i;
    for (int k = 0; k < entries; ++k)
        if (!std::isfinite(m[k])) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: matrix entry %d is not finite", i, k);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(wp.fill[c]))
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: fill of channel %d is not finite", i, c);
    double S[3] = {0, 0, 0};
    for (int r = 0; r < (persp ? 3 : 2); ++r) {
        const double reach = std::fabs((double)m[3 * r]) * wp.out_w + std::fabs((double)m[3 * r + 1]) * wp.out_h +
                             std::fabs((double)m[3 * r + 2]);
        if (reach > kMaxWarpReach)
            return ccmi_set_error(CCMI_ERR_ARG,
                                  "frame %d: matrix row %d reaches %.9g pixels (|m0| out_w + |m1| out_h + |m2| <= 2^22)", i, r,
                                  reach);
        S[r] = reach;
    }
    if (!persp) return CCMI_OK;
    const double eps = 1.0 / 16777216.0; // 2^-24
    double D = 0;
    for (int c = 0; c < 4; ++c) { // the denominator is affine: its minimum over the grid is at a corner pixel centre
        const double v = (double)m[6] * (c & 1 ? wp.out_w - 0.5 : 0.5) + (double)m[7] * (c & 2 ? wp.out_h - 0.5 : 0.5) + (double)m[8];
        if (c == 0 || v < D) D = v;
    }
    const double Dp = D - 3 * eps * S[2];
    if (!(Dp > 0))
        return ccmi_set_error(CCMI_ERR_ARG,
                              "frame %d: the denominator m20 cx + m21 cy + m22 is not positive over the output (%.9g at a corner)",
                              i, D);
    for (int r = 0; r < 2; ++r)
        if (S[r] / Dp > kMaxWarpReach)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: matrix row %d reaches %.9g pixels after the division (<= 2^22)", i, r,
                                  S[r] / Dp);
    for (int r = 0; r < 2; ++r) {
        const double L = (r == 0 ? fw : fh) + 3.0;
        const double E = 3 * eps * (S[r] + L * S[2]) / Dp + 2 * eps * L;
        if (E > 0.875)
            return ccmi_set_error(CCMI_ERR_ARG,
                                  "frame %d: the perspective is too strong for float32 positions (row %d: %.6g pixel, at most 7/8)",
                                  i, r, E);
    }
    return CCMI_OK;
}

// The window of an h x w frame a checked warp samples (the rule is in ccmi.h): the bounding box of
// the taps in double (reach = 1: the bilinear taps x0, x0 + 1; 2: the cubic's x0 - 1 .. x0 + 2), grown
// by one pixel, each end clamped into the frame; even = grown to even x, y, w, h (h and w even).
DecWindow warp_window(const ccmi_warp &wp, int i, int h, int w, bool even, int reach)
{
    const bool persp = (wp.pad & CCMI_WARP_PROJECTIVE) != 0;
    const float *m = wp.matrix + (persp ? 9 : 6) * (size_t)i;
    const double cx[2] = {0.5, wp.out_w - 0.5}, cy[2] = {0.5, wp.out_h - 0.5};
    int end[2][2]; // [axis: x, y][first, last]
    for (int r = 0; r < 2; ++r) {
        double lo = 0, hi = 0;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                double v = (double)m[3 * r] * cx[a] + (double)m[3 * r + 1] * cy[b] + (double)m[3 * r + 2];
                // the image of the rectangle is a convex quadrilateral (the checked denominator is positive): the
                // extremes of the quotient are at the corners too
                if (persp) v /= (double)m[6] * cx[a] + (double)m[7] * cy[b] + (double)m[8];
                if ((a | b) == 0 || v < lo) lo = v;
                if ((a | b) == 0 || v > hi) hi = v;
            }
        const double last = (r == 0 ? w : h) - 1;
        end[r][0] = (int)std::min(std::max(std::floor(lo - 0.5) - reach, 0.0), last);
        end[r][1] = (int)std::min(std::max(std::floor(hi - 0.5) + reach + 1, 0.0), last);
    }
    DecWindow win{end[1][0], end[1][1] + 1, end[0][0], end[0][1] + 1};
    if (even) win = DecWindow{win.y0 & ~1, (win.y1 + 1) & ~1, win.x0 & ~1, (win.x1 + 1) & ~1};
    return win;
}

// A formatted sink (ccmi_tensor_fmt) for the region `rect` of frame i: validates the format
// against the region and resolves it into d; *span = the elements from the frame's first to its
// last, + 1.  of = the sample format tensor_format() chose.  rs (optional): the region is
// resampled, so the frame the strides describe is rs->out_h x rs->out_w; wp (optional, checked):
// the region is the window a warp samples, the frame wp->out_h x wp->out_w.
int tensor_fmt(const ccmi_tensor_fmt &m, const ccmi_resample *rs, const ccmi_warp *wp, int i, const FrameHost &f,
               const OutFmt &of, const DecWindow &rect, DecFmt &d, size_t *span)
{
    if (m.elem != CCMI_ELEM_F32 && m.elem != CCMI_ELEM_F16 && m.elem != CCMI_ELEM_BF16)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: unknown element type %d", i, m.elem);
    if (m.colour != CCMI_COLOUR_ASIS && m.colour != CCMI_COLOUR_RGB)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: unknown colour %d", i, m.colour);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(m.scale[c]) || !std::isfinite(m.bias[c]))
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: scale / bias of channel %d is not finite", i, c);
    if (of.kind == kYuv420 && ((rect.w() | rect.h()) & 1))
        return ccmi_set_error(CCMI_ERR_ARG,
                              "frame %d: a formatted 420 region needs an even size (w %d h %d); out_chroma = 444 takes any",
                              i, rect.w(), rect.h());
    if (rs) {
        if (rs->filter != CCMI_FILTER_TRIANGLE && rs->filter != CCMI_FILTER_CUBIC &&
            rs->filter != (CCMI_FILTER_CUBIC | CCMI_FILTER_CLAMP))
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: unknown filter %d", i, rs->filter);
        if (rs->out_w < 1 || rs->out_w > kMaxResample || rs->out_h < 1 || rs->out_h > kMaxResample)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: output size w %d h %d (1 .. %d)", i, rs->out_w, rs->out_h,
                                  kMaxResample);
        if (rect.w() > kMaxResample || rect.h() > kMaxResample)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: a resampled region is at most %d a side (w %d h %d)", i,
                                  kMaxResample, rect.w(), rect.h());
    }
    // of the stored frame
    const int w = rs ? rs->out_w : wp ? wp->out_w : rect.w(), h = rs ? rs->out_h : wp ? wp->out_h : rect.h();
    int64_t sc = m.stride_c, sy = m.stride_y, sx = m.stride_x;
    if (sc == 0 && sy == 0 && sx == 0) sc = (int64_t)w * h, sy = w, sx = 1;
    const int64_t big = (int64_t)1 << 40; // times an extent (16-bit frame sizes): every product below fits 64 bits
    if (sc < 0 || sy < 0 || sx < 0 || sc >= big || sy >= big || sx >= big)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: strides c %lld y %lld x %lld (elements, 0 .. 2^40)", i,
                              (long long)m.stride_c, (long long)m.stride_y, (long long)m.stride_x);
    // no two elements of the frame at one address: by ascending stride, each dimension steps over
    // the whole of the one before it (a dimension of extent 1 never steps)
    std::pair<int64_t, int64_t> dim[3] = {{sc, 3}, {sy, h}, {sx, w}};
    std::sort(dim, dim + 3);
    int64_t reach = 1; // stride x extent of the widest dimension so far
    for (const auto &[stride, extent] : dim) {
        if (extent == 1) continue;
        if (stride < reach)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: strides c %lld y %lld x %lld let elements of the %d x %d frame alias",
                                  i, (long long)sc, (long long)sy, (long long)sx, w, h);
        reach = stride * extent;
    }
    d = DecFmt{};
    d.on = 1;
    d.elem = m.elem;
    d.matrix = m.colour == CCMI_COLOUR_RGB && f.frame_data_type != 0;
    d.mirror = m.mirror && m.mirror[i];
    for (int c = 0; c < 3; ++c) d.scale[c] = m.scale[c], d.bias[c] = m.bias[c];
    d.stride_c = sc, d.stride_y = sy, d.stride_x = sx;
    if (rs) {
        d.rs = 1, d.out_h = h, d.out_w = w;
        d.cubic = (rs->filter & 0xff) == CCMI_FILTER_CUBIC, d.clamp = (rs->filter & CCMI_FILTER_CLAMP) != 0;
    }
    if (wp) {
        d.warp = 1, d.out_h = h, d.out_w = w, d.pad = wp->pad & 1;
        d.cubic = (wp->pad & CCMI_WARP_CUBIC) != 0, d.clamp = (wp->pad & CCMI_WARP_CLAMP) != 0;
        d.persp = (wp->pad & CCMI_WARP_PROJECTIVE) != 0;
        for (int c = 0; c < 3; ++c) d.fill[c] = wp->fill[c];
        const int stride = d.persp ? 9 : 6;
        for (int k = 0; k < stride; ++k) d.m[k] = wp->matrix[stride * (size_t)i + k];
    }
    *span = (size_t)(2 * sc + (h - 1) * sy + (w - 1) * sx + 1);
    return CCMI_OK;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ccmi_colour of frame i, whose ops start at `first` of the flat array: validated and resolved into d
// (1 - f in float32 here, once; a factor of -0 becomes +0).
int colour_ops(const ccmi_colour &cl, int i, size_t first, DecCol &d)
{
    const int n = cl.count[i];
    if (n < 0 || n > CCMI_COL_MAX_OPS)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: %d colour ops (0 .. %d)", i, n, CCMI_COL_MAX_OPS);
    d = DecCol{};
    d.n = n;
    for (int k = 0; k < n; ++k) {
        const ccmi_colour_op &op = cl.ops[first + k];
        DecColOp &o = d.ops[k];
        o.op = op.op;
        switch (op.op) {
        case CCMI_COL_MATRIX:
            for (int e = 0; e < 12; ++e) {
                if (!std::isfinite(op.v[e]))
                    return ccmi_set_error(CCMI_ERR_ARG, "frame %d: colour op %d: matrix entry %d is not finite", i, k, e);
                o.v[e] = op.v[e];
            }
            break;
        case CCMI_COL_CONTRAST:
            if (d.contrast >= 0)
                return ccmi_set_error(CCMI_ERR_ARG, "frame %d: colour ops %d and %d are both contrast ops (at most one)", i,
                                      d.contrast, k);
            d.contrast = k;
            [[fallthrough]];
        case CCMI_COL_BRIGHTNESS:
        case CCMI_COL_SATURATION:
            if (!std::isfinite(op.v[0]) || op.v[0] < 0.f)
                return ccmi_set_error(CCMI_ERR_ARG, "frame %d: colour op %d: factor %g (finite, >= 0)", i, k, (double)op.v[0]);
            o.v[0] = op.v[0] + 0.f;
            o.v[1] = 1.f - o.v[0];
            break;
        default:
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: colour op %d: unknown op %d", i, k, op.op);
        }
    }
    return CCMI_OK;
}

// ccmi_filter of frame i, whose half taps start at `first` of the flat array: validated and resolved
// into d; *takes = the frame takes the stage
int filter_frame(const ccmi_filter &fl, int i, size_t first, DecFlt &d, bool *takes)
{
    const int r = fl.radius[i];
    if (r < 0 || r > CCMI_FLT_MAX_RADIUS)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: blur radius %d (0 .. %d)", i, r, CCMI_FLT_MAX_RADIUS);
    d = DecFlt{};
    d.r = r;
    if (r > 0) {
        if (!fl.taps) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: blur taps are NULL", i);
        for (int k = 0; k <= r; ++k) {
            if (!std::isfinite(fl.taps[first + k]))
                return ccmi_set_error(CCMI_ERR_ARG, "frame %d: blur tap %d is not finite", i, k);
            d.taps[k] = fl.taps[first + k];
        }
    }
    if (fl.solarize) {
        const float th = fl.solarize[i];
        if (std::isnan(th)) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: solarize threshold is NaN", i);
        d.sol = th <= 1.0f;
        d.th = th;
    }
    *takes = r > 0 || d.sol;
    return CCMI_OK;
}

// ccmi_mix of frame i of n, whose rectangles start at `first` of the flat array: everything that needs no
// stored size, validated and resolved (1 - lam) into d
int mix_frame(const ccmi_mix &mx, int i, int n, size_t first, DecMix &d)
{
    d = DecMix{};
    const int cnt = mx.count ? mx.count[i] : 0;
    if (cnt < 0 || cnt > CCMI_MIX_MAX_RECTS)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: %d erase rectangles (0 .. %d)", i, cnt, CCMI_MIX_MAX_RECTS);
    if (cnt > 0 && !mx.rects) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: erase rectangles are NULL", i);
    d.count = cnt;
    d.seed = mx.seed ? mx.seed[i] : 0;
    for (int k = 0; k < cnt; ++k) {
        const ccmi_erase_rect &q = mx.rects[first + k];
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(q.v[c]))
                return ccmi_set_error(CCMI_ERR_ARG, "frame %d: erase rectangle %d: value %d is not finite", i, k, c);
        if (!std::isfinite(q.sigma) || q.sigma < 0.f)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: erase rectangle %d: sigma %g (finite, >= 0)", i, k, (double)q.sigma);
        if (q.w < 0 || q.h < 0)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: erase rectangle %d: negative size (w %d h %d)", i, k, q.w, q.h);
        d.r[k] = DecMixRect{q.x, q.y, q.w, q.h, {q.v[0], q.v[1], q.v[2]}, q.sigma};
    }
    const int p = mx.partner ? mx.partner[i] : -1;
    if (p < -1 || p >= n) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: partner %d (-1, or a frame 0 .. %d)", i, p, n - 1);
    d.partner = p;
    const ccmi_rect b = mx.box ? mx.box[i] : ccmi_rect{0, 0, 0, 0};
    if (b.w < 0 || b.h < 0) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: mix box of negative size (w %d h %d)", i, b.w, b.h);
    if (p < 0) return CCMI_OK;
    if (b.w > 0 && b.h > 0) { // CutMix: lam is not read
        d.box[0] = b.x, d.box[1] = b.y, d.box[2] = b.w, d.box[3] = b.h;
        return CCMI_OK;
    }
    if (!mx.lam) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: lam is NULL", i);
    const float lam = mx.lam[i];
    if (!(lam >= 0.f && lam <= 1.f)) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: lam %g (in [0, 1])", i, (double)lam);
    d.lam = lam, d.oml = 1.0f - lam;
    return CCMI_OK;
}

// the rest of frame i's ccmi_mix, once every frame's stored size oh[] x ow[] is known: non-empty
// rectangles and boxes inside the frame, and a partner of the frame's size
int mix_frame_sized(const DecMix &d, int i, const std::vector<int> &oh, const std::vector<int> &ow)
{
    const auto inside = [&](int x, int y, int w, int h) {
        return x >= 0 && y >= 0 && w <= ow[i] && h <= oh[i] && x <= ow[i] - w && y <= oh[i] - h;
    };
    for (int k = 0; k < d.count; ++k) {
        const DecMixRect &q = d.r[k];
        if (q.w > 0 && q.h > 0 && !inside(q.x, q.y, q.w, q.h))
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: erase rectangle %d (x %d y %d w %d h %d) outside the %d x %d frame", i,
                                  k, q.x, q.y, q.w, q.h, ow[i], oh[i]);
    }
    if (d.partner < 0) return CCMI_OK;
    if (d.box[2] > 0 && !inside(d.box[0], d.box[1], d.box[2], d.box[3]))
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: mix box (x %d y %d w %d h %d) outside the %d x %d frame", i, d.box[0],
                              d.box[1], d.box[2], d.box[3], ow[i], oh[i]);
    if (oh[d.partner] != oh[i] || ow[d.partner] != ow[i])
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: partner %d is stored at %d x %d, the frame at %d x %d", i, d.partner,
                              ow[d.partner], oh[d.partner], ow[i], oh[i]);
    return CCMI_OK;
}

// ccmi_blend of frame i of n, whose terms start at `first` of the flat arrays: everything that needs no
// stored size, validated into d; mx: the frame's resolved ccmi_mix, or NULL
int blend_frame(const ccmi_blend &bl, int i, int n, size_t first, const DecMix *mx, DecBlend &d)
{
    d = DecBlend{};
    const int cnt = bl.count ? bl.count[i] : 0;
    if (cnt < 0 || cnt > CCMI_BLEND_MAX_TERMS)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: %d blend terms (0 .. %d)", i, cnt, CCMI_BLEND_MAX_TERMS);
    if (cnt > 0 && (!bl.source || !bl.weight))
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: blend %s are NULL", i, bl.source ? "weights" : "sources");
    d.count = cnt;
    d.silent = bl.silent && bl.silent[i] ? 1 : 0;
    for (int t = 0; t < cnt; ++t) {
        const int q = bl.source[first + t];
        const float w = bl.weight[first + t];
        if (q < 0 || q >= n)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: blend term %d: source %d (a frame 0 .. %d)", i, t, q, n - 1);
        if (!std::isfinite(w)) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: blend term %d: weight is not finite", i, t);
        d.src[t] = q, d.w[t] = w;
    }
    if (d.silent && (cnt > 0 || (mx && (mx->count > 0 || mx->partner >= 0))))
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: a silent frame with %s (it writes no output)", i,
                              cnt > 0 ? "blend terms" : mx->count > 0 ? "erase rectangles" : "a partner");
    return CCMI_OK;
}

// ccmi_tone of frame i, whose ops start at `first` of the flat array: validated, resolved (1 - f, the
// posterize levels) and cut into segments in d
int tone_ops(const ccmi_tone &tn, int i, size_t first, DecTone &d)
{
    const int n = tn.count[i];
    if (n < 0 || n > CCMI_TONE_MAX_OPS)
        return ccmi_set_error(CCMI_ERR_ARG, "frame %d: %d tone ops (0 .. %d)", i, n, CCMI_TONE_MAX_OPS);
    d = DecTone{};
    d.n = n;
    int seg_first = 0, src = 0, acc = 0;
    auto close = [&](int end, int term) {
        DecToneSeg &g = d.seg[d.nseg++];
        g.first = (uint8_t)seg_first, g.end = (uint8_t)end, g.term = (uint8_t)term, g.src = (uint8_t)src, g.acc = (uint8_t)acc;
        seg_first = end + 1;
    };
    for (int k = 0; k < n; ++k) {
        const ccmi_tone_op &op = tn.ops[first + k];
        DecToneOp &o = d.ops[k];
        o.op = op.op;
        switch (op.op) {
        case CCMI_TONE_MATRIX:
            for (int e = 0; e < 12; ++e) {
                if (!std::isfinite(op.v[e]))
                    return ccmi_set_error(CCMI_ERR_ARG, "frame %d: tone op %d: matrix entry %d is not finite", i, k, e);
                o.v[e] = op.v[e];
            }
            break;
        case CCMI_TONE_BRIGHTNESS:
        case CCMI_TONE_SATURATION:
        case CCMI_TONE_CONTRAST:
        case CCMI_TONE_SHARPNESS:
            if (!std::isfinite(op.v[0]) || op.v[0] < 0.f)
                return ccmi_set_error(CCMI_ERR_ARG, "frame %d: tone op %d: factor %g (finite, >= 0)", i, k, (double)op.v[0]);
            o.v[0] = op.v[0] + 0.f;
            o.v[1] = 1.f - o.v[0];
            break;
        case CCMI_TONE_SOLARIZE:
            if (std::isnan(op.v[0])) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: tone op %d: solarize threshold is NaN", i, k);
            o.v[0] = op.v[0];
            break;
        case CCMI_TONE_POSTERIZE: {
            const float b = op.v[0];
            if (!(b >= 1.f && b <= 8.f) || b != (float)(int)b)
                return ccmi_set_error(CCMI_ERR_ARG, "frame %d: tone op %d: posterize bits %g (an integer in 1 .. 8)", i, k,
                                      (double)b);
            const float L = (float)(1 << (int)b);
            o.v[0] = L, o.v[1] = 1.0f / L, o.v[2] = L - 1.f;
            break;
        }
        case CCMI_TONE_AUTOCONTRAST:
        case CCMI_TONE_EQUALIZE:
            break;
        default:
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: tone op %d: unknown op %d", i, k, op.op);
        }
        if (op.op == CCMI_TONE_SHARPNESS) {
            close(k, op.op);
            src ^= 1; // the later passes read the other buffer
        } else if (op.op == CCMI_TONE_CONTRAST || op.op == CCMI_TONE_AUTOCONTRAST || op.op == CCMI_TONE_EQUALIZE) {
            close(k, op.op);
            ++acc;
        }
    }
    if (seg_first < n) close(n, kToneNoTerm);
    return CCMI_OK;
}

// the architecture part of a frame's tail arguments (no device pointers): what
// dec_tail_batchable() looks at, the true plane sizes and the workspace sizes
void tail_arch(const FrameHost &f, DecTailFrame &t)
{
    DecUpsArgs &ua = t.ups;
    ua = DecUpsArgs{};
    ua.n_layers = f.n_layers;
    for (int l = 0; l < f.n_layers; ++l) {
        ua.lh[l] = f.lh[l];
        ua.lw[l] = f.lw[l];
    }
    ua.ups_ks = f.ups_ks;
    ua.n_ups = f.n_ups;
    ua.pre_ks = f.pre_ks;
    ua.n_pre = f.n_pre;
    DecSynArgs &sa = t.syn;
    sa = DecSynArgs{};
    sa.c_in = f.n_layers;
    sa.h = f.h;
    sa.w = f.w;
    sa.n_layers = (int)f.layers.size();
    for (int l = 0; l < sa.n_layers; ++l) sa.layers[l] = f.layers[l];
}

// A device sink's region, output format and tail mode; fills rq.geom[i] / rq.info[i].
int plan_tensor_sink(const DecodeRequest &rq, int i, FramePlan &p)
{
    const FrameHost &f = p.f;
    DecTailFrame &t = p.tail;
    size_t elems = 0;
    DecWindow rect{0, f.h, 0, f.w};
    const char *who = rq.src ? "frame" : "stream"; // a render's outputs are frames of the handle's streams
    if (rq.roi) {
        const ccmi_rect &q = rq.roi[i];
        if (q.w < 1 || q.h < 1 || q.x < 0 || q.y < 0 || q.x > f.w - q.w || q.y > f.h - q.h)
            return ccmi_set_error(CCMI_ERR_ARG, "%s %d: region x %d y %d w %d h %d outside the %d x %d frame", who, i,
                                  q.x, q.y, q.w, q.h, f.w, f.h);
        rect = DecWindow{q.y, q.y + q.h, q.x, q.x + q.w};
    }
    if (rq.warp) { // the region is the window the matrix reaches
        if (int rc = warp_check(*rq.warp, i, f.h, f.w)) return rc;
        rect = warp_window(*rq.warp, i, f.h, f.w, false, rq.warp->pad & CCMI_WARP_CUBIC ? 2 : 1);
    }
    if (int rc = tensor_format(f, rq.out_bitdepth, rq.out_chroma, rq.sample, p.of, &elems, rect)) {
        if (!rq.src) return rc;
        std::string m = ccmi_last_error();
        return ccmi_set_error(rc, "frame %d: %s", i, m.c_str());
    }
    if (rq.warp && p.of.kind == kYuv420) {
        if ((f.w | f.h) & 1)
            return ccmi_set_error(
                CCMI_ERR_ARG, "frame %d: a warp of 420 samples needs an even frame size (w %d h %d); out_chroma = 444 takes any",
                i, f.w, f.h);
        rect = warp_window(*rq.warp, i, f.h, f.w, true, rq.warp->pad & CCMI_WARP_CUBIC ? 2 : 1);
    }
    if (rq.window) rq.window[i] = ccmi_rect{rect.x0, rect.y0, rect.w(), rect.h()};
    if (p.of.kind == kYuv420 && ((rect.x0 | rect.y0) & 1))
        return ccmi_set_error(CCMI_ERR_ARG, "%s %d: a 420 region needs an even origin (x %d y %d)", who, i, rect.x0,
                              rect.y0);
    size_t unit = sample_bytes(rq.sample); // bytes of one stored element
    int out_w = rect.w(), out_h = rect.h();  // of the stored frame: the region, unless it is resampled
    if (rq.fmt) {
        size_t span = 0;
        if (int rc = tensor_fmt(*rq.fmt, rq.rs, rq.warp, i, f, p.of, rect, t.fmt, &span)) return rc;
        unit = elem_bytes(t.fmt.elem);
        elems = 3 * (size_t)rect.h() * rect.w();
        if (t.fmt.rs) {
            out_w = t.fmt.out_w, out_h = t.fmt.out_h;
            elems = 3 * (size_t)out_h * out_w;
            p.rs_elems = dec_resample_tmp_elems(rect.h(), out_w);
        }
        if (t.fmt.warp) {
            out_w = t.fmt.out_w, out_h = t.fmt.out_h;
            elems = 3 * (size_t)out_h * out_w;
        }
        p.of.payload = span * unit; // what the caller's buffer must hold
    }
    int halo = 0;
    for (const SynLayerDesc &L : f.layers) halo += (L.ks - 1) / 2;
    if (rect.h() == f.h && rect.w() == f.w) {
        p.mode = kTailFrame;
    } else if (p.batchable) {
        p.mode = kTailWindow;
        dec_roi_plan(f.lh, f.lw, f.n_layers, f.ups_ks, f.pre_ks, halo, rect, t.roi);
    } else {
        p.mode = kTailCrop;
    }
    if (p.mode != kTailWindow) { // the whole frame is decoded
        dec_roi_plan(f.lh, f.lw, f.n_layers, f.ups_ks, f.pre_ks, halo, DecWindow{0, f.h, 0, f.w}, t.roi);
        t.roi.rect = rect;
    }
    t.windowed = p.mode == kTailWindow;
    if (rq.geom)
        rq.geom[i] = ccmi_frame_geom{out_w, out_h, p.of.bitdepth, p.of.kind == kYuv420 ? 420 : 444,
                                     f.frame_data_type, elems};
    if (rq.info) {
        ccmi_roi_info &I = rq.info[i];
        I = ccmi_roi_info{};
        I.n_grids = f.n_layers;
        for (int l = 0; l < f.n_layers; ++l) I.arm_rows[l] = t.roi.arm_rows[l];
        I.windowed = p.batchable ? 1 : 0;
    }
    if (rq.dev && !p.silent) { // ccmi_blend: nothing is written for a silent frame, its output is not looked at
        if (!rq.dev[i]) return ccmi_set_error(CCMI_ERR_ARG, "decode: output %d is NULL", i);
        if (reinterpret_cast<uintptr_t>(rq.dev[i]) % unit)
            return ccmi_set_error(CCMI_ERR_ARG, "decode: output %d is not aligned to its %zu-byte samples", i, unit);
    }
    return CCMI_OK;
}

// Stream i: header, sink format, region, capacity -- in this order, which fixes the first
// error an input reports.
int plan_frame(const DecodeRequest &rq, int i, FramePlan &p)
{
    if (rq.src) { // the header facts and the networks come from the handle: nothing is parsed or decoded
        const int n_src = (int)rq.src->s.size();
        p.src = rq.index ? rq.index[i] : i;
        if (p.src < 0 || p.src >= n_src)
            return ccmi_set_error(CCMI_ERR_ARG, "frame %d: index %d outside the handle's %d streams", i, p.src, n_src);
        p.f = rq.src->s[p.src].f;
    } else {
        if (!rq.streams[i]) return ccmi_set_error(CCMI_ERR_ARG, "decode: stream %d is NULL", i);
        if (int rc = parse_frame_header(rq.streams[i], rq.lens[i], p.f)) {
            std::string m = ccmi_last_error();
            return ccmi_set_error(rc, "stream %d: %s", i, m.c_str());
        }
    }
    const FrameHost &f = p.f;
    DecTailFrame &t = p.tail;
    tail_arch(f, t);
    if (rq.src) t.syn.f24 = rq.src->s[p.src].f24;
    p.batchable = f.n_branches == 1 && dec_tail_batchable(t);
    if (rq.device()) {
        if (int rc = plan_tensor_sink(rq, i, p)) return rc;
    } else if (rq.lat_store) { // no tail, no output: every latent row
        for (int l = 0; l < f.n_layers; ++l) t.roi.arm_rows[l] = f.lh[l];
    } else {
        if (int rc = out_format(f, rq.out_bitdepth, rq.out_chroma, rq.as_yuv, p.of)) return rc;
        for (int l = 0; l < f.n_layers; ++l) t.roi.arm_rows[l] = f.lh[l];
    }
    // the pack kernel loads its sources 16 bytes at a time: a store build starts every plane on 4 values
    const int plane_align = rq.lat_store ? 4 : 1;
    p.lat_elems = 0;
    for (int l = 0, off = 0; l < f.n_layers; ++l) {
        t.ups.off[l] = off;
        off += (t.roi.arm_rows[l] * f.lw[l] + plane_align - 1) / plane_align * plane_align;
        p.lat_elems = (size_t)off;
    }
    t.bitdepth = p.of.bitdepth;
    t.kind = p.of.kind;
    t.sample = rq.sample;
    const size_t bytes = p.of.header + p.of.payload;
    if ((rq.outs || rq.dev) && rq.caps && !p.silent && rq.caps[i] < bytes)
        return ccmi_set_error(CCMI_ERR_ARG, "%s %d: output buffer of %zu bytes, need %zu", rq.src ? "frame" : "stream", i,
                              rq.caps[i], bytes);
    if (rq.sizes) rq.sizes[i] = bytes;
    return CCMI_OK;
}

// One device allocation: the constant part (coded bytes + weights, uploaded in one copy),
// then every frame's scratch, then the call's tables.
void plan_layout(const DecodeRequest &rq, DecodePlan &pl)
{
    // A render from a latent store has no constant part (the tail reads the networks from the
    // store), no ARM descriptors and no status words; a store build has no tail scratch.
    const bool render = rq.src != nullptr, build = rq.lat_store != nullptr;
    size_t cst = 0;
    for (FramePlan &p : pl.fr) {
        if (render) break;
        const FrameHost &f = p.f;
        for (int l = 0; l < f.n_layers; ++l) {
            p.bytes_off[l] = cst;
            cst += align_up(f.lat_n[l] + 64, 256);
        }
        p.arm_off = cst;
        cst += align_up(f.arm.size() * 4, 256);
        p.ups_off = cst;
        cst += align_up(f.ups.size() * 4, 256);
        p.syn_off = cst;
        cst += align_up(f.syn.size() * 4, 256);
    }
    pl.cst = cst;
    size_t tot = align_up(cst, 4096);
    for (FramePlan &p : pl.fr) {
        const FrameHost &f = p.f;
        p.lat_off = tot;
        tot += align_up(p.lat_elems * 4, 256);
        if (build) continue;
        // a region decode on windows: the latent planes keep their frame pitch and hold the rows
        // the ARM decode produces, the pyramid stacks and the synthesis output hold the windows
        const DecRoi &R = p.tail.roi;
        const bool win = p.mode == kTailWindow;
        p.ws_elems = win ? dec_ups_workspace_elems_win(R, f.n_layers) : dec_ups_workspace_elems(f.lh, f.lw, f.n_layers);
        p.dense_elems = win ? (size_t)f.n_layers * R.lev[0].h() * R.lev[0].w() : (size_t)f.n_layers * f.h * f.w;
        p.synout_elems = win ? (size_t)f.layers.back().n_out * R.rect.h() * R.rect.w()
                             : (size_t)f.layers.back().n_out * f.h * f.w * f.n_branches;
        p.synws_elems = dec_syn_workspace_elems(p.tail.syn);
        p.ws_off = tot;
        tot += align_up(p.ws_elems * 4 + 4, 256);
        p.dense_off = tot;
        tot += align_up(p.dense_elems * 4, 256);
        p.synout_off = tot;
        tot += align_up(p.synout_elems * 4, 256);
        p.synws_off = tot;
        tot += align_up(p.synws_elems * 4 + 4, 256);
        if (p.rs_elems) {
            p.rs_off = tot;
            tot += align_up(p.rs_elems * 4, 256);
        }
        if (p.flt_elems) {
            p.flt_off = tot;
            tot += align_up(p.flt_elems * 4, 256);
            if (!pl.tones.empty() && dec_tone_sharps(pl.tones[&p - pl.fr.data()])) {
                p.tone2_off = tot;
                tot += align_up(p.flt_elems * 4, 256);
            }
            if (p.tail.mix && dec_flt_class(p.tail) == 1) { // ccmi_mix: the filter kernel's float32 output
                p.mix2_off = tot;
                tot += align_up(p.flt_elems * 4, 256);
            }
        }
        p.out_off = tot;
        if (!rq.device()) tot += align_up(p.of.payload, 256); // device sinks write to the caller's memory
    }
    pl.desc_off = tot;
    if (!render) tot += align_up(sizeof(ArmStreamDesc) * pl.n_status(), 256);
    // batched-tail argument tables: bounded by one single-frame table per frame
    pl.tail_cap = 0;
    for (const FramePlan &p : pl.fr)
        if (!build)
            pl.tail_cap += dec_tail_table_bytes(p.f.n_layers, 1, p.mode == kTailWindow, dec_out_form(p.tail.fmt), pl.col);
    pl.tail_off = tot;
    tot += align_up(pl.tail_cap, 256);
    // the pack / unpack job table follows the tail tables: one host image, one upload.  A build
    // has a job per grid and two more per stream (the networks' integers), a render one per grid.
    pl.lat_tab_off = tot;
    pl.lat_tab_cap = 0;
    for (const FramePlan &p : pl.fr)
        pl.lat_tab_cap += build ? sizeof(DecLatPackJob) * (size_t)(p.f.n_layers + 2)
                                : render ? sizeof(DecLatUnpackJob) * (size_t)p.f.n_layers : 0;
    tot += align_up(pl.lat_tab_cap, 256);
    // the filter stage's tables follow the job table in the same host image: the same upload
    pl.flt_tab_off = tot;
    tot += pl.flt_table_bytes();
    pl.mix_tab_off = tot; // ccmi_mix: the mix table ends the image
    tot += pl.mix_table_bytes();
    pl.blend_tab_off = tot; // ccmi_blend: ... or its sibling, the blend table
    tot += pl.blend_table_bytes();
    if (!pl.tones.empty()) { // ccmi_tone: the accumulator blocks of the call's statistic ops, frame after frame
        pl.tone_acc_off = tot;
        for (size_t i = 0; i < pl.fr.size(); ++i) {
            pl.fr[i].tone_acc_off = tot;
            tot += kToneAccBytes * (size_t)dec_tone_stats(pl.tones[i]);
        }
        pl.tone_acc_bytes = tot - pl.tone_acc_off;
    }
    pl.col_off = tot;
    if (pl.col) tot += align_up(sizeof(unsigned long long) * pl.fr.size(), 256);
    pl.status_off = tot;
    if (!render) tot += align_up(4 * pl.n_status(), 256);
#if defined(CCMI_ARM_STAMPS)
    pl.dbg_off = tot;
    tot += align_up(16 * 8 * pl.n_status(), 256);
#endif
    pl.total = tot;
}

} // namespace

int decode_plan(const DecodeRequest &rq, DecodePlan &pl)
{
    if (rq.n < 1) return ccmi_set_error(CCMI_ERR_ARG, rq.src ? "render: no frames (m < 1)" : "decode: no streams");
    if (rq.src && !rq.index && rq.n != (int)rq.src->s.size())
        return ccmi_set_error(CCMI_ERR_ARG, "render: %d frames without an index, the handle has %zu streams", rq.n,
                              rq.src->s.size());
    if (rq.rs && rq.warp)
        return ccmi_set_error(CCMI_ERR_ARG, "frame 0: a resample and a warp are both given (a call takes one geometry)");
    if (rq.warp && rq.roi)
        return ccmi_set_error(CCMI_ERR_ARG, "frame 0: a warp takes no roi (the matrix says where the output lies)");
    pl = DecodePlan{};
    pl.fr.resize(rq.n);
    if (rq.colour) { // every frame's ops first: whether any frame has one decides the form of the whole call
        if (!rq.fmt || !rq.colour->count)
            return ccmi_set_error(CCMI_ERR_ARG, "frame 0: colour without %s", rq.fmt ? "its counts" : "a format");
        size_t first = 0;
        pl.cols.resize(rq.n);
        for (int i = 0; i < rq.n; ++i) {
            if (rq.colour->count[i] > 0 && !rq.colour->ops) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: colour ops are NULL", i);
            DecCol &d = pl.cols[i];
            if (int rc = colour_ops(*rq.colour, i, first, d)) return rc;
            first += (size_t)d.n;
            pl.col = pl.col || d.n > 0;
            pl.col_stat = pl.col_stat || d.contrast >= 0;
        }
    }
    if (!pl.col) pl.cols.clear(); // no op in any frame: the call without colour
    std::vector<char> takes; // ccmi_filter: the frames that take the stage
    if (rq.filter) { // every frame's filter next: a rejected one is reported before any frame is planned
        if (!rq.fmt || !rq.filter->radius)
            return ccmi_set_error(CCMI_ERR_ARG, "frame 0: a filter without %s", rq.fmt ? "its radii" : "a format");
        size_t first = 0;
        pl.flts.resize(rq.n);
        takes.assign(rq.n, 0);
        for (int i = 0; i < rq.n; ++i) {
            bool t = false;
            if (int rc = filter_frame(*rq.filter, i, first, pl.flts[i], &t)) return rc;
            if (pl.flts[i].r > 0) first += (size_t)pl.flts[i].r + 1;
            takes[i] = t;
            pl.n_flt += t;
        }
    }
    if (rq.tone) { // every frame's tone list: a frame with one takes the stage too
        if (!rq.fmt || !rq.tone->count)
            return ccmi_set_error(CCMI_ERR_ARG, "frame 0: tone ops without %s", rq.fmt ? "their counts" : "a format");
        size_t first = 0;
        bool any = false;
        pl.tones.resize(rq.n);
        for (int i = 0; i < rq.n; ++i) {
            if (rq.tone->count[i] > 0 && !rq.tone->ops) return ccmi_set_error(CCMI_ERR_ARG, "frame %d: tone ops are NULL", i);
            if (int rc = tone_ops(*rq.tone, i, first, pl.tones[i])) return rc;
            first += (size_t)pl.tones[i].n;
            any = any || pl.tones[i].n > 0;
        }
        if (!any) pl.tones.clear(); // no op in any frame: the call without tone
        if (any) {
            if (takes.empty()) takes.assign(rq.n, 0);
            // a frame staged by its tone ops alone is formatted by the filter kernel: radius 0, no solarize
            pl.flts.resize(rq.n);
            for (int i = 0; i < rq.n; ++i)
                if (pl.tones[i].n > 0 && !takes[i]) takes[i] = 1, ++pl.n_flt;
        }
    }
    if (rq.mix) { // every frame's rectangles, partner and weights: the mix-staged frames take the stage too
        if (!rq.fmt) return ccmi_set_error(CCMI_ERR_ARG, "frame 0: mix without a format");
        size_t first = 0;
        bool any = false;
        pl.mixes.resize(rq.n);
        for (int i = 0; i < rq.n; ++i) {
            if (int rc = mix_frame(*rq.mix, i, rq.n, first, pl.mixes[i])) return rc;
            first += (size_t)pl.mixes[i].count;
            any = any || pl.mixes[i].count > 0 || pl.mixes[i].partner >= 0;
        }
        if (!any) pl.mixes.clear(); // no frame takes the stage: the call without mix
        if (any) {
            for (int i = 0; i < rq.n; ++i)
                if (pl.mixes[i].count > 0 || pl.mixes[i].partner >= 0) {
                    pl.mixes[i].staged = 1;
                    if (pl.mixes[i].partner >= 0) pl.mixes[pl.mixes[i].partner].staged = 1;
                }
        }
    }
    if (rq.blend) { // every frame's terms and silence: the blend-staged frames are mix-staged
        if (!rq.fmt) return ccmi_set_error(CCMI_ERR_ARG, "frame 0: blend without a format");
        size_t first = 0;
        bool any = false;
        pl.blends.resize(rq.n);
        for (int i = 0; i < rq.n; ++i) {
            const DecMix *mx = pl.mixes.empty() ? nullptr : &pl.mixes[i];
            if (int rc = blend_frame(*rq.blend, i, rq.n, first, mx, pl.blends[i])) return rc;
            first += (size_t)pl.blends[i].count;
            any = any || pl.blends[i].count > 0 || pl.blends[i].silent;
        }
        if (!any) pl.blends.clear(); // no frame has terms or is silent: the call without blend
        if (any) {
            if (pl.mixes.empty()) pl.mixes.assign(rq.n, DecMix{});
            for (int i = 0; i < rq.n; ++i) {
                const DecBlend &b = pl.blends[i];
                pl.fr[i].silent = b.silent != 0;
                if (b.count > 0 || b.silent) pl.mixes[i].staged = 1;
                for (int t = 0; t < b.count; ++t) pl.mixes[b.src[t]].staged = 1;
            }
        }
    }
    if (!pl.mixes.empty()) {
        if (takes.empty()) takes.assign(rq.n, 0);
        // a frame staged for the mix alone passes the filter stage with radius 0 and no solarize
        pl.flts.resize(rq.n);
        for (int i = 0; i < rq.n; ++i) {
            if (!pl.mixes[i].staged) continue;
            pl.mixes[i].entry = pl.n_mix++;
            if (!takes[i]) takes[i] = 1, ++pl.n_flt;
        }
    }
    if (!pl.n_flt) pl.flts.clear(); // no frame takes the stage: the call without a filter
    std::vector<int> oh(rq.n, 0), ow(rq.n, 0); // the stored sizes
    for (int i = 0; i < rq.n; ++i) {
        FramePlan &p = pl.fr[i];
        if (int rc = plan_frame(rq, i, p)) return rc;
        p.tail.fmt.col = pl.col ? 1 : 0;
        p.tail.col = pl.col ? &pl.cols[i] : nullptr;
        const DecFmt &d = p.tail.fmt;
        const bool sized = d.rs || d.warp;
        oh[i] = sized ? d.out_h : p.tail.roi.rect.h(), ow[i] = sized ? d.out_w : p.tail.roi.rect.w();
        if (pl.n_flt && takes[i]) { // staged at the size of the stored frame
            p.tail.flt = &pl.flts[i];
            if (!pl.tones.empty()) p.tail.tone = &pl.tones[i];
            if (pl.n_mix && pl.mixes[i].staged) p.tail.mix = &pl.mixes[i];
            p.flt_elems = 3 * (size_t)oh[i] * (size_t)ow[i];
        }
    }
    for (int i = 0; i < rq.n && pl.n_mix; ++i)
        if (int rc = mix_frame_sized(pl.mixes[i], i, oh, ow)) return rc;
    for (size_t i = 0; i < pl.blends.size(); ++i) // a source is read at the frame's own (c, i, k)
        for (int t = 0; t < pl.blends[i].count; ++t) {
            const int q = pl.blends[i].src[t];
            if (oh[q] != oh[i] || ow[q] != ow[i])
                return ccmi_set_error(CCMI_ERR_ARG,
                                      "frame %zu: blend term %d: source %d is stored at %d x %d, the frame at %d x %d", i, t, q,
                                      ow[q], oh[q], ow[i], oh[i]);
        }
    plan_layout(rq, pl);
    return CCMI_OK;
}

int latent_store_layout(const DecodePlan &pl, int type, ccmi_latents &h)
{
    if (type == CCMI_LATENT_SEG)
        return ccmi_set_error(CCMI_ERR_ARG,
                              "latents: a CCMI_LATENT_SEG store has a data-dependent size and is not built from streams: "
                              "build an I8 / I16 / I32 store, then ccmi_latents_compact_measure / ccmi_latents_compact");
    const size_t eb = dec_lat_elem_bytes(type);
    if (!eb) return ccmi_set_error(CCMI_ERR_ARG, "latents: unknown element type %d", type);
    h.s.resize(pl.fr.size());
    size_t pos = 0;
    for (size_t i = 0; i < pl.fr.size(); ++i) {
        const FrameHost &f = pl.fr[i].f;
        LatentStream &S = h.s[i];
        S.type = type;
        S.off = pos;
        S.ups_off = pos;
        pos += align_up(f.ups.size() * 4, 16);
        S.syn_off = pos;
        pos += align_up(f.syn.size() * 4, 16);
        for (int l = 0; l < f.n_layers; ++l) {
            S.grid_off[l] = pos;
            if (f.lat_n[l]) pos += align_up((size_t)f.lh[l] * f.lw[l] * eb, 16);
        }
        pos = align_up(pos, 256);
        S.bytes = pos - S.off;
    }
    h.store_bytes = pos;
    return CCMI_OK;
}

} // namespace ccmi
