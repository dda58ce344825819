// dist_msssim.hip -- multi-scale SSIM distortion on the device: value and gradient for batches of
// frames (ccmi_msssim_f32) and, through ccmi_launch_msssim, the overfit step's second distortion
// term (train.hip, ccmi_train_step_dist).  The contract is in include/ccmi.h; tests/msssim_ref.py
// restates it in torch.
//
//   ms_pool    one launch per scale s >= 1: clamp (scale 1 only) and 2x2-mean X and Y into the workspace
//   ms_stat    one launch: per (frame, plane, scale, tile of kTH x kTW outputs) stage the tile's
//              (kTH + 10) x (kTW + 10) samples of X - 1/2 and Y - 1/2 in LDS, window the five products
//              horizontally, then vertically, form cs and l, write ONE partial sum per workgroup and,
//              with a gradient, the three derivative maps (d / d mu_x, d / d G*(XX), d / d G*(XY))
//   ms_reduce  one workgroup per frame: the partials of every (plane, scale) in a fixed order, v_s,
//              MS_p, MS, MSE, D and the gradient factors
//   ms_grad    one launch per scale, coarsest first: the transposed window over the three maps (same
//              two LDS passes), times the factor, plus a quarter of the parent's gradient; scale 0
//              adds the MSE term, applies the clamp mask and stores through the plane's addressing
//
// The derivative maps are STORED by ms_stat and read back by ms_grad (12 bytes per output position
// and scale) rather than recomputed: recomputing needs the tile's statistics on a halo of 10 more
// positions per side, (42 x 52) / (22 x 32) = 3.1 x the window work of a tile, against one write and 1.9 reads.
#include "ccmi_internal.h"

#include <cmath>

namespace {

constexpr int kT = 256;
constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kTH = 22, kTW = 32;                   // outputs per tile
constexpr int kSR = kTH + kHalo, kSC = kTW + kHalo; // staged samples per tile: 32 x 42
constexpr int kSP = kSC + 1;                        // staged row pitch: the horizontal pass's 4 rows x 8 segments of a
                                                    // half wave fall on 32 different banks
constexpr int kHP = kTW + 1;                        // pitch of the horizontally windowed rows, likewise
constexpr int kMaxP = 3, kMaxS = 5;
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;
static_assert(kSR * (kTW / 4) == kT, "the horizontal pass gives each thread one row segment of 4 outputs");
static_assert(kTH <= 3 * (kT / kTW), "the vertical pass gives each thread 3 rows of one column");

struct MsWin {
    float g[kWin];
};

struct MsGeo {
    int P, S;
    int h[kMaxP][kMaxS], w[kMaxP][kMaxS];
    int tile0[kMaxP][kMaxS];    // first statistics tile of (p, s) among the frame's tiles_per
    int64_t pyr_off[kMaxP][kMaxS]; // float offset of (p, s >= 1) in a frame's pyramid block
    int64_t map_off[kMaxP][kMaxS]; // float offset of (p, s) in a frame's block of one derivative map
    int64_t y_off[kMaxP];       // float offset of plane p in a packed frame of Y
    int64_t pyr_per, map_per;
    int tiles_per;
    float total;                // samples of every plane of a frame
};

// where plane p of X at scale 0 lives (ccmi_msssim_args.x / grad)
struct MsSrc {
    int64_t stride, off[kMaxP], pitch[kMaxP];
    int sub[kMaxP];
    int clamp;
};

__host__ __device__ __forceinline__ int div_up(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// fixed-order tree over the workgroup's kT values
__device__ __forceinline__ float block_tree(float v, float *s_red)
{
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int n = kT / 2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) s_red[threadIdx.x] += s_red[threadIdx.x + n];
        __syncthreads();
    }
    return s_red[0];
}

// ---------------------------------------------------------------- pyramid
// scale s -> s + 1 of X and Y of every plane: avg_pool2d(2, padding = size mod 2, count_include_pad)
__global__ __launch_bounds__(kT) void ms_pool(MsGeo g, int s, MsSrc src, const float *__restrict__ x,
                                              const float *__restrict__ y, int64_t y_stride, float *__restrict__ pyrX,
                                              float *__restrict__ pyrY)
{
    const int b = blockIdx.y, p = blockIdx.z;
    const int h = g.h[p][s], w = g.w[p][s], hn = g.h[p][s + 1], wn = g.w[p][s + 1];
    const int ph = h & 1, pw = w & 1;
    const float *xs, *ys;
    int64_t xr, yr = w;
    int xc, cl;
    if (s == 0) {
        xs = x + (int64_t)b * src.stride + src.off[p];
        xr = (int64_t)src.sub[p] * src.pitch[p];
        xc = src.sub[p];
        cl = src.clamp;
        ys = y + (int64_t)b * y_stride + g.y_off[p];
    } else {
        xs = pyrX + (int64_t)b * g.pyr_per + g.pyr_off[p][s];
        xr = w;
        xc = 1;
        cl = 0;
        ys = pyrY + (int64_t)b * g.pyr_per + g.pyr_off[p][s];
    }
    float *xo = pyrX + (int64_t)b * g.pyr_per + g.pyr_off[p][s + 1];
    float *yo = pyrY + (int64_t)b * g.pyr_per + g.pyr_off[p][s + 1];
    const int n = hn * wn;
    for (int e = blockIdx.x * kT + threadIdx.x; e < n; e += gridDim.x * kT) {
        const int i = e / wn, j = e - i * wn;
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int ii = 2 * i - ph + a, jj = 2 * j - pw + c;
                if (ii >= 0 && jj >= 0 && ii < h && jj < w) { // ii < h, jj < w always hold; kept as the bound
                    float xv = xs[ii * xr + (int64_t)jj * xc];
                    if (cl) xv = clamp01(xv);
                    sx += xv;
                    sy += ys[ii * yr + jj];
                }
            }
        xo[e] = 0.25f * sx;
        yo[e] = 0.25f * sy;
    }
}

// ---------------------------------------------------------------- the two window passes
// horizontal: thread t takes row t / 8, outputs 4 (t % 8) .. + 3 of NQ staged planes -> sH[q]
// vertical:   thread t takes column t % 32, output rows 3 (t / 32) .. + 2 -> acc[q][o]
template <int NQ, class F>
__device__ __forceinline__ void win_h(const MsWin &W, float *__restrict__ sH, F &&prod)
{
    const int row = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    float acc[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[q][c] = 0.f;
#pragma unroll
    for (int k = 0; k < 4 + kHalo; ++k) {
        float v[NQ];
        prod(row * kSP + c4 + k, v);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (k - c >= 0 && k - c < kWin) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q][c] = fmaf(W.g[k - c], v[q], acc[q][c]);
            }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) sH[q * kSR * kHP + row * kHP + c4 + c] = acc[q][c];
}

template <int NQ>
__device__ __forceinline__ void win_v(const MsWin &W, const float *__restrict__ sH, float (&acc)[NQ][3])
{
    const int col = threadIdx.x & (kTW - 1), r3 = (threadIdx.x >> 5) * 3;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int o = 0; o < 3; ++o) acc[q][o] = 0.f;
#pragma unroll
    for (int k = 0; k < 3 + kHalo; ++k) {
        const int rr = r3 + k;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float v = rr < kSR ? sH[q * kSR * kHP + rr * kHP + col] : 0.f; // rows past the tile feed no kept output
#pragma unroll
            for (int o = 0; o < 3; ++o)
                if (k - o >= 0 && k - o < kWin) acc[q][o] = fmaf(W.g[k - o], v, acc[q][o]);
        }
    }
}

// ---------------------------------------------------------------- statistics
// part: [B][tiles_per][2] = the tile's sum of cs (cs l at the last scale), and at scale 0 the squared
// error of the samples the tile owns; maps: 3 x [B][map_per] or null
__global__ __launch_bounds__(kT) void ms_stat(MsGeo g, MsWin W, MsSrc src, const float *__restrict__ x,
                                              const float *__restrict__ y, int64_t y_stride,
                                              const float *__restrict__ pyrX, const float *__restrict__ pyrY,
                                              float *__restrict__ maps, int64_t map_plane, float *__restrict__ part)
{
    __shared__ float sX[kSR * kSP], sY[kSR * kSP], sH[5 * kSR * kHP];
    const int b = blockIdx.y, tile = blockIdx.x;
    int p = 0, s = 0;
    for (int pp = 0; pp < g.P; ++pp)
        for (int ss = 0; ss < g.S; ++ss)
            if (tile >= g.tile0[pp][ss]) p = pp, s = ss; // tile0 ascends in (p, s) order
    const int h = g.h[p][s], w = g.w[p][s], oh = h - kHalo, ow = w - kHalo;
    const int ntx = div_up(ow, kTW), nty = div_up(oh, kTH);
    const int t = tile - g.tile0[p][s], ty = t / ntx, tx = t - ty * ntx;
    const int r0 = ty * kTH, c0 = tx * kTW;
    const float *xs, *ys;
    int64_t xr;
    int xc, cl;
    if (s == 0) {
        xs = x + (int64_t)b * src.stride + src.off[p];
        xr = (int64_t)src.sub[p] * src.pitch[p];
        xc = src.sub[p];
        cl = src.clamp;
        ys = y + (int64_t)b * y_stride + g.y_off[p];
    } else {
        xs = pyrX + (int64_t)b * g.pyr_per + g.pyr_off[p][s];
        xr = w;
        xc = 1;
        cl = 0;
        ys = pyrY + (int64_t)b * g.pyr_per + g.pyr_off[p][s];
    }
    // stage; the last tile of a row / column of tiles owns the 10 halo samples too (MSE)
    float se = 0.f;
    for (int e = threadIdx.x; e < kSR * kSC; e += kT) {
        const int r = e / kSC, c = e - r * kSC;
        const int gi = r0 + r, gj = c0 + c;
        float xv = 0.5f, yv = 0.5f;
        if (gi < h && gj < w) {
            xv = xs[gi * xr + (int64_t)gj * xc];
            if (cl) xv = clamp01(xv);
            yv = ys[(int64_t)gi * w + gj];
            if (s == 0 && (r < kTH || ty == nty - 1) && (c < kTW || tx == ntx - 1)) {
                const float d = xv - yv;
                se = fmaf(d, d, se);
            }
        }
        sX[r * kSP + c] = xv - 0.5f;
        sY[r * kSP + c] = yv - 0.5f;
    }
    __syncthreads();
    win_h<5>(W, sH, [&](int at, float (&v)[5]) {
        const float a = sX[at], c = sY[at];
        v[0] = a, v[1] = c, v[2] = a * a, v[3] = c * c, v[4] = a * c;
    });
    __syncthreads();
    float m[5][3];
    win_v<5>(W, sH, m);
    const int col = threadIdx.x & (kTW - 1), r3 = (threadIdx.x >> 5) * 3;
    const bool last = s == g.S - 1;
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const int li = r3 + o, gi = r0 + li, gj = c0 + col;
        if (li < kTH && gi < oh && gj < ow) {
            const float ax = m[0][o], ay = m[1][o]; // means of X - 1/2, Y - 1/2
            const float sxx = m[2][o] - ax * ax, syy = m[3][o] - ay * ay, sxy = m[4][o] - ax * ay;
            const float dc = sxx + syy + kC2, cs = (2.f * sxy + kC2) / dc;
            const float mx = ax + 0.5f, my = ay + 0.5f;
            const float dl = mx * mx + my * my + kC1, l = last ? (2.f * mx * my + kC1) / dl : 1.f;
            sum += cs * l;
            if (maps) {
                // f = cs l: d f / d s_xx, d f / d s_xy, and d f / d mu_x through s_xx, s_xy and l
                const float db = -l * cs / dc, dcv = 2.f * l / dc;
                float da = -2.f * ax * db - ay * dcv;
                if (last) da += cs * (2.f * my - 2.f * mx * l) / dl;
                float *mp = maps + (int64_t)b * g.map_per + g.map_off[p][s] + (int64_t)gi * ow + gj;
                mp[0] = da;
                mp[map_plane] = db;
                mp[2 * map_plane] = dcv;
            }
        }
    }
    float *red = sH; // every read of sH is behind block_tree's first barrier
    const float tot = block_tree(sum, red);
    const float tse = s == 0 ? block_tree(se, red) : 0.f;
    if (threadIdx.x == 0) {
        float *o = part + ((int64_t)b * g.tiles_per + tile) * 2;
        o[0] = tot;
        o[1] = tse;
    }
}

// ---------------------------------------------------------------- reduction
struct MsComb {
    float weights[kMaxS], cw[kMaxP], alpha, beta;
};

// out: [B][4] = D, MS, MSE, min v_s;  fac: [B][16], entry p * 5 + s = - beta cw_p w_s MS_p / v_s / n_s
__global__ __launch_bounds__(kT) void ms_reduce(MsGeo g, MsComb c, const float *__restrict__ part,
                                                float *__restrict__ out, float *__restrict__ fac)
{
    __shared__ float s_red[kT];
    const int b = blockIdx.x;
    const float *pb = part + (int64_t)b * g.tiles_per * 2;
    float ms = 0.f, se = 0.f, vmin = INFINITY;
    for (int p = 0; p < g.P; ++p) {
        float v[kMaxS], msp = 1.f;
        bool dead = false;
        for (int s = 0; s < g.S; ++s) {
            const int oh = g.h[p][s] - kHalo, ow = g.w[p][s] - kHalo;
            const int nt = div_up(oh, kTH) * div_up(ow, kTW);
            const float *q = pb + (int64_t)g.tile0[p][s] * 2;
            float a = 0.f, e = 0.f;
            for (int i = threadIdx.x; i < nt; i += kT) {
                a += q[2 * i];
                e += q[2 * i + 1];
            }
            a = block_tree(a, s_red);
            if (s == 0) se += block_tree(e, s_red);
            v[s] = a / ((float)oh * (float)ow);
            vmin = fminf(vmin, v[s]);
            if (v[s] <= 0.f) dead = true;
            else msp *= powf(v[s], c.weights[s]);
        }
        if (dead) msp = 0.f;
        ms = fmaf(c.cw[p], msp, ms);
        if (threadIdx.x == 0)
            for (int s = 0; s < g.S; ++s) {
                const float n = (float)(g.h[p][s] - kHalo) * (float)(g.w[p][s] - kHalo);
                fac[b * 16 + p * kMaxS + s] = dead ? 0.f : -c.beta * c.cw[p] * c.weights[s] * msp / v[s] / n;
            }
    }
    if (threadIdx.x == 0) {
        const float mse = se / g.total;
        out[b * 4 + 0] = c.alpha * mse + c.beta * (1.f - ms);
        out[b * 4 + 1] = ms;
        out[b * 4 + 2] = mse;
        out[b * 4 + 3] = vmin;
    }
}

// ---------------------------------------------------------------- gradient
// scale s of every plane, tiles of kTH x kTW SAMPLES: g_s = fac (T(a) + 2 (X - 1/2) T(b) + (Y - 1/2) T(c))
// + 1/4 g_{s+1}(parent); a is d / d mu_x of the shifted statistics, so the shifted samples go with it
__global__ __launch_bounds__(kT) void ms_grad(MsGeo g, MsWin W, int s, MsSrc src, const float *__restrict__ x,
                                              const float *__restrict__ y, int64_t y_stride,
                                              const float *__restrict__ pyrX, const float *__restrict__ pyrY,
                                              const float *__restrict__ maps, int64_t map_plane,
                                              const float *__restrict__ fac, float k_mse, float *__restrict__ gpyr,
                                              float *__restrict__ grad)
{
    __shared__ float sM[3][kSR * kSP], sH[3 * kSR * kHP];
    const int b = blockIdx.y;
    int tile = blockIdx.x, p = 0;
    for (; p < g.P - 1; ++p) {
        const int n = div_up(g.h[p][s], kTH) * div_up(g.w[p][s], kTW);
        if (tile < n) break;
        tile -= n;
    }
    const int h = g.h[p][s], w = g.w[p][s], oh = h - kHalo, ow = w - kHalo;
    const int ntx = div_up(w, kTW), ty = tile / ntx, tx = tile - ty * ntx;
    const int r0 = ty * kTH, c0 = tx * kTW;
    const float *mp = maps + (int64_t)b * g.map_per + g.map_off[p][s];
    for (int e = threadIdx.x; e < kSR * kSC; e += kT) {
        const int r = e / kSC, c = e - r * kSC;
        const int mi = r0 - kHalo + r, mj = c0 - kHalo + c; // map position; sample i takes positions i - 10 .. i
        float a = 0.f, bb = 0.f, cc = 0.f;
        if (mi >= 0 && mj >= 0 && mi < oh && mj < ow) {
            const float *q = mp + (int64_t)mi * ow + mj;
            a = q[0], bb = q[map_plane], cc = q[2 * map_plane];
        }
        sM[0][r * kSP + c] = a;
        sM[1][r * kSP + c] = bb;
        sM[2][r * kSP + c] = cc;
    }
    __syncthreads();
    win_h<3>(W, sH, [&](int at, float (&v)[3]) { v[0] = sM[0][at], v[1] = sM[1][at], v[2] = sM[2][at]; });
    __syncthreads();
    float m[3][3];
    win_v<3>(W, sH, m); // the window is symmetric: the transposed pass is the same pass over the shifted stage
    const int col = threadIdx.x & (kTW - 1), r3 = (threadIdx.x >> 5) * 3;
    const float f = fac[b * 16 + p * kMaxS + s];
    const bool top = s == g.S - 1;
    const int ph = h & 1, pw = w & 1;
    const int wn = top ? 0 : g.w[p][s + 1];
    const float *gn = top ? nullptr : gpyr + (int64_t)b * g.pyr_per + g.pyr_off[p][s + 1];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const int li = r3 + o, gi = r0 + li, gj = c0 + col;
        if (li < kTH && gi < h && gj < w) {
            if (s == 0) {
                const int64_t at = (int64_t)b * src.stride + src.off[p] + gi * ((int64_t)src.sub[p] * src.pitch[p]) +
                                   (int64_t)gj * src.sub[p];
                const float raw = x[at], xv = src.clamp ? clamp01(raw) : raw;
                const float yv = y[(int64_t)b * y_stride + g.y_off[p] + (int64_t)gi * w + gj];
                float gv = f * (m[0][o] + 2.f * (xv - 0.5f) * m[1][o] + (yv - 0.5f) * m[2][o]);
                if (!top) gv = fmaf(0.25f, gn[(int64_t)((gi + ph) >> 1) * wn + ((gj + pw) >> 1)], gv);
                gv = fmaf(k_mse, xv - yv, gv);
                if (src.clamp && !(raw >= 0.f && raw <= 1.f)) gv = 0.f;
                grad[at] = gv;
            } else {
                const int64_t at = (int64_t)b * g.pyr_per + g.pyr_off[p][s] + (int64_t)gi * w + gj;
                const float xv = pyrX[at], yv = pyrY[at];
                float gv = f * (m[0][o] + 2.f * (xv - 0.5f) * m[1][o] + (yv - 0.5f) * m[2][o]);
                if (!top) gv = fmaf(0.25f, gn[(int64_t)((gi + ph) >> 1) * wn + ((gj + pw) >> 1)], gv);
                gpyr[at] = gv;
            }
        }
    }
}

// ---------------------------------------------------------------- host
size_t al256(size_t floats) { return (floats * sizeof(float) + 255) / 256 * 256; }

struct MsPlan {
    MsGeo g;
    size_t pyrX, pyrY, part, fac, gpyr, maps, total; // byte offsets into the workspace
};

// every argument check that needs no device; CCMI_OK fills pl
int ms_plan(const ccmi_msssim_args *a, MsPlan &pl)
{
    if (!a) return ccmi_set_error(CCMI_ERR_ARG, "msssim: null argument");
    if (a->batch < 1 || a->batch > 65535) return ccmi_set_error(CCMI_ERR_ARG, "msssim: batch %d outside 1 .. 65535", a->batch);
    if (a->n_planes < 1 || a->n_planes > kMaxP) return ccmi_set_error(CCMI_ERR_ARG, "msssim: n_planes %d outside 1 .. 3", a->n_planes);
    if (a->n_scales < 1 || a->n_scales > kMaxS) return ccmi_set_error(CCMI_ERR_ARG, "msssim: n_scales %d outside 1 .. 5", a->n_scales);
    for (int s = 0; s < a->n_scales; ++s)
        if (!std::isfinite(a->weights[s]) || a->weights[s] < 0.f)
            return ccmi_set_error(CCMI_ERR_ARG, "msssim: weights[%d] is negative or not finite", s);
    for (int p = 0; p < a->n_planes; ++p)
        if (!std::isfinite(a->channel_weights[p]) || a->channel_weights[p] < 0.f)
            return ccmi_set_error(CCMI_ERR_ARG, "msssim: channel_weights[%d] is negative or not finite", p);
    if (!std::isfinite(a->alpha_mse) || !std::isfinite(a->beta_ms) || a->alpha_mse < 0.f || a->beta_ms < 0.f)
        return ccmi_set_error(CCMI_ERR_ARG, "msssim: alpha_mse / beta_ms is negative or not finite");
    MsGeo &g = pl.g;
    g = MsGeo{};
    g.P = a->n_planes;
    g.S = a->n_scales;
    int64_t pyr = 0, map = 0, yo = 0, tiles = 0;
    for (int p = 0; p < g.P; ++p) {
        if (a->x_sub[p] != 1 && a->x_sub[p] != 2)
            return ccmi_set_error(CCMI_ERR_ARG, "msssim: x_sub[%d] = %d, must be 1 or 2", p, a->x_sub[p]);
        if (a->h[p] < 1 || a->w[p] < 1 || a->h[p] > (1 << 15) || a->w[p] > (1 << 15))
            return ccmi_set_error(CCMI_ERR_ARG, "msssim: plane %d is %d x %d", p, a->h[p], a->w[p]);
        if (a->x_off[p] < 0 || a->x_pitch[p] < (int64_t)(a->w[p] - 1) * a->x_sub[p] + 1)
            return ccmi_set_error(CCMI_ERR_ARG, "msssim: plane %d: x_off < 0 or x_pitch below a row of samples", p);
        int h = a->h[p], w = a->w[p];
        g.y_off[p] = yo;
        yo += (int64_t)h * w;
        for (int s = 0; s < g.S; ++s) {
            if (h < kWin || w < kWin)
                return ccmi_set_error(CCMI_ERR_ARG, "msssim: plane %d is %d x %d at scale %d, below the 11 x 11 window", p, h, w, s);
            g.h[p][s] = h;
            g.w[p][s] = w;
            g.tile0[p][s] = (int)tiles;
            tiles += (int64_t)div_up(h - kHalo, kTH) * div_up(w - kHalo, kTW);
            g.map_off[p][s] = map;
            map += (int64_t)(h - kHalo) * (w - kHalo);
            g.pyr_off[p][s] = s ? pyr : 0;
            if (s) pyr += (int64_t)h * w;
            h = (h + 1) / 2;
            w = (w + 1) / 2;
        }
    }
    g.pyr_per = pyr;
    g.map_per = map;
    g.tiles_per = (int)tiles;
    g.total = (float)yo;
    const size_t B = (size_t)a->batch;
    size_t o = 0;
    pl.pyrX = o, o += al256(B * pyr);
    pl.pyrY = o, o += al256(B * pyr);
    pl.part = o, o += al256(2 * B * tiles);
    pl.fac = o, o += al256(16 * B);
    pl.gpyr = pl.maps = o;
    if (a->grad) {
        pl.gpyr = o, o += al256(B * pyr);
        pl.maps = o, o += al256(3 * B * map);
    }
    pl.total = o;
    return CCMI_OK;
}

int ms_check_ptrs(const ccmi_msssim_args *a, const MsPlan &pl)
{
    if (!a->out) return ccmi_set_error(CCMI_ERR_ARG, "msssim: out is null");
    if (!a->x || !a->y) return ccmi_set_error(CCMI_ERR_ARG, "msssim: x or y is null");
    if (a->y_stride != 0 && a->y_stride < (int64_t)pl.g.total)
        return ccmi_set_error(CCMI_ERR_ARG, "msssim: y_stride %lld below a frame's %lld samples (0: one shared target)",
                              (long long)a->y_stride, (long long)pl.g.total);
    if (!a->workspace || a->workspace_bytes < pl.total)
        return ccmi_set_error(CCMI_ERR_ARG, "msssim: workspace of %zu bytes needed", pl.total);
    return CCMI_OK;
}

MsWin ms_window()
{
    double t[kWin], sum = 0.0;
    for (int k = 0; k < kWin; ++k) sum += t[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5);
    MsWin W;
    for (int k = 0; k < kWin; ++k) W.g[k] = (float)(t[k] / sum);
    return W;
}

} // namespace

extern "C" size_t ccmi_msssim_workspace_bytes(const ccmi_msssim_args *a)
{
    MsPlan pl;
    if (ms_plan(a, pl)) return 0;
    return pl.total;
}

int ccmi_msssim_check(const ccmi_msssim_args *a)
{
    MsPlan pl;
    if (int rc = ms_plan(a, pl)) return rc;
    return ms_check_ptrs(a, pl);
}

int ccmi_launch_msssim(const ccmi_msssim_args *a, hipStream_t st)
{
    MsPlan pl;
    if (int rc = ms_plan(a, pl)) return rc;
    if (int rc = ms_check_ptrs(a, pl)) return rc;
    const MsGeo &g = pl.g;
    const int B = a->batch;
    uint8_t *ws = static_cast<uint8_t *>(a->workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    float *pyrX = F(pl.pyrX), *pyrY = F(pl.pyrY), *part = F(pl.part), *fac = F(pl.fac);
    float *gpyr = a->grad ? F(pl.gpyr) : nullptr, *maps = a->grad ? F(pl.maps) : nullptr;
    const int64_t map_plane = (int64_t)B * g.map_per;
    MsSrc src{};
    src.stride = a->x_stride;
    src.clamp = a->clamp ? 1 : 0;
    for (int p = 0; p < g.P; ++p) {
        src.off[p] = a->x_off[p];
        src.pitch[p] = a->x_pitch[p];
        src.sub[p] = a->x_sub[p];
    }
    const MsWin W = ms_window();
    for (int s = 0; s + 1 < g.S; ++s) {
        int n = 0;
        for (int p = 0; p < g.P; ++p) n = std::max(n, g.h[p][s + 1] * g.w[p][s + 1]);
        hipLaunchKernelGGL(ms_pool, dim3((unsigned)std::min(div_up(n, kT), 1024), B, g.P), dim3(kT), 0, st, g, s, src,
                           a->x, a->y, a->y_stride, pyrX, pyrY);
    }
    hipLaunchKernelGGL(ms_stat, dim3((unsigned)g.tiles_per, B), dim3(kT), 0, st, g, W, src, a->x, a->y, a->y_stride, pyrX,
                       pyrY, maps, map_plane, part);
    MsComb c{};
    for (int s = 0; s < g.S; ++s) c.weights[s] = a->weights[s];
    for (int p = 0; p < g.P; ++p) c.cw[p] = a->channel_weights[p];
    c.alpha = a->alpha_mse;
    c.beta = a->beta_ms;
    hipLaunchKernelGGL(ms_reduce, dim3(B), dim3(kT), 0, st, g, c, part, a->out, fac);
    if (a->grad)
        for (int s = g.S - 1; s >= 0; --s) {
            int n = 0;
            for (int p = 0; p < g.P; ++p) n += div_up(g.h[p][s], kTH) * div_up(g.w[p][s], kTW);
            hipLaunchKernelGGL(ms_grad, dim3((unsigned)n, B), dim3(kT), 0, st, g, W, s, src, a->x, a->y, a->y_stride, pyrX,
                               pyrY, maps, map_plane, fac, a->alpha_mse * 2.f / g.total, gpyr, a->grad);
        }
    CCMI_HIP_CHECK(hipGetLastError());
    return CCMI_OK;
}

extern "C" int ccmi_msssim_f32(const ccmi_msssim_args *a, void *stream)
{
    if (int rc = ccmi_msssim_check(a)) return rc; // before any HIP call
    return ccmi_launch_msssim(a, static_cast<hipStream_t>(stream));
}
