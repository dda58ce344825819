// dec_mix_entry.h -- path B: what the kernels of the mix stage (dec_mix.hip) and of the blend stage
// (dec_blend.hip) share: the tile and the entry of the call's mix table.
// Everything is internal to the including file.
#pragma once

#include "ccmi_noise.h"
#include "dec_out_fmt.h"

namespace ccmi {
namespace {

constexpr int kThreads = kOutThreads;
constexpr int kTileH = 16;             // rows of a tile
constexpr int kTileG = 16;             // groups of 4 destination pixels per tile row
static_assert(kThreads == kTileH * kTileG, "one group per thread");

// one mix-staged frame (DecMix with its device pointers): kMixTableBytes of the call's mix table
struct DecMixEntry {
    const float *src; // [3][oh][ow], the frame as it will be stored (mirrored already), before step 4
    void *dst;
    unsigned long long seed;
    int oh, ow;
    int partner; // the partner's entry, or -1
    int count;
    float lam, oml;
    int bx, by, bw, bh; // bw == 0: no box
    DecMixRect r[CCMI_MIX_MAX_RECTS];
    // the frame's own resolved strides (elements): all-zero strides in ccmi_tensor_fmt resolve to each
    // frame's stored size, and the mix-staged frames of one call may differ in size
    long long sc, sy, sx;
    int terms; // ccmi_blend: the frame's terms in its entry of the blend table; 0: the frame itself
    int pad_[9];
};
static_assert(sizeof(DecMixEntry) == kMixTableBytes, "the mix entry of kMixTableBytes");

typedef float __attribute__((address_space(1))) GlobalFloat;

// the tile's pixel rectangle [x0, x1) x [y0, y1) against the rectangle (x, y, w, h)
__device__ __forceinline__ bool meets(int x0, int x1, int y0, int y1, int x, int y, int w, int h)
{
    return w > 0 && h > 0 && x < x1 && x + w > x0 && y < y1 && y + h > y0;
}

int mix_tiles_x(int ow) { return (fmt_row_groups(ow) + kTileG - 1) / kTileG; }
int mix_tiles_y(int oh) { return (oh + kTileH - 1) / kTileH; }

} // namespace
} // namespace ccmi
