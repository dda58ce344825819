"""The host side of the bicubic forms (CCMI_FILTER_CUBIC / CCMI_FILTER_CLAMP of ccmi_resample,
CCMI_WARP_CUBIC / CCMI_WARP_CLAMP or'ed into ccmi_warp.pad): which values the plan takes, and what
a cubic plan shares with the bilinear plan of the same call.  As tests/test_decode_resample_abi.py
and tests/test_decode_warp_abi.py: no compute, the plan calls make no GPU call, and the run entry
points are only ever called with arguments the plan rejects."""
import ctypes as C
import math

import numpy as np
import pytest

import cubic_ref as R
import warp_ref as W
import test_decode_resample_abi as RA
import test_decode_warp_abi as WA
from test_decode_resample_abi import E_BF16, E_F16, Geom, Handle, Info, Rect, Rs, _fields, _first, _fmt, _is_arg_error
from test_decode_warp_abi import IDENT, ccmi_frame

FILTER_TRIANGLE, FILTER_CUBIC, FILTER_CLAMP = 0, 2, 0x100
PAD_FILL, PAD_EDGE, WARP_CUBIC, WARP_CLAMP = 0, 1, 0x100, 0x200
FILTERS_OK = (0, 2, 0x102)
FILTERS_BAD = (1, 3, 0x100, 0x202, -1, 77)
PADS_OK = (0, 1, 0x100, 0x101, 0x300, 0x301)
PADS_BAD = (2, 0x200, 0x201, 0x400, -1, 77)


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    P, I, Z = RA.P, RA.I, RA.Z
    lib.ccmi_decode_batch_dev_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_decode_batch_dev_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_rs.argtypes = [P, P, I, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_warp.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_latents_render_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
    lib.ccmi_latents_render_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for f in (lib.ccmi_decode_batch_dev_fmt_plan, lib.ccmi_decode_batch_dev_rs_plan, lib.ccmi_decode_batch_dev_rs,
              lib.ccmi_decode_batch_dev_warp_plan, lib.ccmi_decode_batch_dev_warp, lib.ccmi_latents_decode,
              lib.ccmi_latents_render_rs_plan, lib.ccmi_latents_render_warp_plan, lib.ccmi_decode_last_tail_groups):
        f.restype = C.c_int
    return lib


def _groups(lib):
    a, b = C.c_int(7), C.c_int(7)
    assert lib.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


# ------------------------------------------------------------------ accepted and rejected values
def test_filter_values(L, data):
    import ccmi
    rects = [(352, 176, 64, 32), (1024, 464, 256, 200)]
    for filt in FILTERS_OK:
        rc, geom, _, need = RA._plan(L, data[:2], rects, _fmt(), Rs(32, 24, filt))
        assert rc == 0 and need > 0, (filt, ccmi.last_error())
        assert (geom[1].width, geom[1].height) == (32, 24)
    for filt in FILTERS_BAD:
        rc, _, _, got = RA._plan(L, data[:2], rects, _fmt(), Rs(32, 24, filt))
        _is_arg_error(rc, 0, "filter", str(filt))
        assert got == 0
        rc = RA._run(L, data[:2], rects, _fmt(), Rs(32, 24, filt), [1 << 30] * 2)
        _is_arg_error(rc, 0, "filter")


def test_pad_values(L, data):
    import ccmi
    for pad in PADS_OK:
        w, keep = WA._warp([IDENT] * 2, 8, 8, pad)
        rc, geom, _, win, need = WA._plan(L, data[:2], _fmt(), w, chroma=444)
        assert rc == 0 and need > 0, (pad, ccmi.last_error())
    for pad in PADS_BAD:
        WA._rejected(L, data[:2], [IDENT] * 2, 8, 8, 0, "pad", str(pad), pad=pad)


def test_the_range_checks_hold_for_the_cubic_forms(L, data):
    """Output sizes and region sides: the triangle's limits, 16384 accepted and 16385 refused."""
    import ccmi
    for filt in (2, 0x102):
        for ow, oh in ((16384, 1), (1, 16384)):
            rc, geom, _, _ = RA._plan(L, data[:1], [(0, 0, 64, 64)], _fmt(), Rs(ow, oh, filt))
            assert rc == 0, ccmi.last_error()
        for ow, oh in ((0, 8), (8, 16385)):
            rc, *_ = RA._plan(L, data[:1], [(0, 0, 64, 64)], _fmt(), Rs(ow, oh, filt))
            _is_arg_error(rc, 0, "output size", "16384")
        wide = [RA._header_only(64, 20000)]
        rc, *_ = RA._plan(L, wide, [(0, 0, 16384, 64)], _fmt(), Rs(1, 1, filt))
        assert rc == 0, ccmi.last_error()
        rc, *_ = RA._plan(L, wide, [(0, 0, 16386, 64)], _fmt(), Rs(1, 1, filt))
        _is_arg_error(rc, 0, "16384", "region")
    for pad in (0x100, 0x301):
        WA._rejected(L, data[:2], [IDENT] * 2, 16385, 8, 0, "output size", "16384", pad=pad)
        WA._rejected(L, data, [IDENT, (float("nan"),) * 6, IDENT], 8, 8, 1, "finite", pad=pad)
        WA._rejected(L, data[:2], [IDENT, (1, 0, 2.0 ** 23, 0, 1, 0)], 8, 8, 1, "2^22", pad=pad)


# ------------------------------------------------------------------ the cubic plan against the bilinear plan
def test_cubic_resize_plan_is_the_triangle_plan(L, data):
    """The same geometry, ccmi_roi_info and workspace: only the weights differ."""
    import ccmi
    rects = [(352, 176, 64, 32), (1024, 464, 256, 200), (1, 3, 255, 77)]
    for (ow, oh), chroma in (((224, 224), 0), ((7, 5), 444), ((300, 1), 0)):
        base = RA._plan(L, data, rects, _fmt(E_F16), Rs(ow, oh, 0), chroma=chroma)
        assert base[0] == 0, ccmi.last_error()
        assert _groups(L) == (0, 0)
        for filt in (2, 0x102):
            got = RA._plan(L, data, rects, _fmt(E_F16), Rs(ow, oh, filt), chroma=chroma)
            assert got[0] == 0, ccmi.last_error()
            assert got[3] == base[3]
            assert [_fields(g) for g in got[1]] == [_fields(g) for g in base[1]]
            for a, b in zip(got[2], base[2]):
                assert list(a.arm_rows) == list(b.arm_rows) and (a.windowed, a.n_grids) == (b.windowed, b.n_grids)
            assert _groups(L) == (0, 0)  # a call that only plans launches nothing, whatever its filter
    with Handle(L, data) as H:
        m = 3
        idx, arr = (C.c_int * m)(2, 0, 1), RA._rects([rects[2], rects[0], rects[1]], m)
        f = _fmt(E_BF16)
        needs = []
        for filt in FILTERS_OK:
            rs, geom, need = Rs(96, 64, filt), (Geom * m)(), C.c_size_t(0)
            rc = L.ccmi_latents_render_rs_plan(H.h, idx, m, arr, 0, 444, C.byref(f), C.byref(rs), geom, None, C.byref(need))
            assert rc == 0, ccmi.last_error()
            needs.append((need.value, [_fields(g) for g in geom]))
        assert needs[0] == needs[1] == needs[2]
        bad, geom, need = Rs(96, 64, 0x100), (Geom * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_rs_plan(H.h, idx, m, arr, 0, 444, C.byref(f), C.byref(bad), geom, None, C.byref(need))
        _is_arg_error(rc, 0, "filter")


def test_cubic_windows_follow_the_rule_and_size_the_workspace(L, data):
    """50 random matrices per stream, size and pad: window[] is cubic_ref.window() -- the rule of ccmi.h
    recomputed here with 2 / 3 in place of 1 / 2 --, holds every in-frame tap of the 16, is never
    smaller than the bilinear window of the same matrix, and sizes the workspace as the _fmt plan with
    roi = window does (but for the argument table, as in test_decode_warp_abi.py)."""
    import ccmi
    rng = np.random.default_rng(78)
    for i, stream in enumerate(data):
        H, W_, chroma = ccmi_frame(L, stream)
        for oh, ow in ((224, 224), (17, 39), (1, 1)):
            n = 50
            mats = WA._random_matrices(rng, n, H, W_, oh, ow)
            for pad in (PAD_FILL, PAD_EDGE):
                w, keep = WA._warp(mats, ow, oh, pad, (0.1, 0.2, 0.3))
                rc, _, _, bwin, _ = WA._plan(L, [stream] * n, _fmt(E_BF16), w)
                assert rc == 0, ccmi.last_error()
                wins = {}
                for flags in (WARP_CUBIC, WARP_CUBIC | WARP_CLAMP):
                    w, keep = WA._warp(mats, ow, oh, pad | flags, (0.1, 0.2, 0.3))
                    rc, geom, info, win, need = WA._plan(L, [stream] * n, _fmt(E_BF16), w)
                    assert rc == 0, ccmi.last_error()
                    wins[flags] = win
                    for j, m in enumerate(mats):
                        x, y, ww, hh = win[j]
                        assert win[j] == R.window(m, oh, ow, H, W_, even=chroma == 420), (i, j)
                        assert bwin[j] == R.window(m, oh, ow, H, W_, even=chroma == 420, reach=1) == \
                            W.window(m, oh, ow, H, W_, even=chroma == 420)
                        bx, by, bw, bh = bwin[j]
                        assert x <= bx and y <= by and x + ww >= bx + bw and y + hh >= by + bh, (i, j)
                        assert ww >= 1 and hh >= 1 and x >= 0 and y >= 0 and x + ww <= W_ and y + hh <= H
                        if chroma == 420:
                            assert (x | y | ww | hh) & 1 == 0
                        ty, tx = R.taps_in_frame(m, oh, ow, H, W_)
                        assert not ((tx < x) | (tx >= x + ww) | (ty < y) | (ty >= y + hh)).any(), (i, j)
                        assert (geom[j].width, geom[j].height, geom[j].elems) == (ow, oh, 3 * ow * oh)
                    rc, _, finfo, fneed = WA._plan_fmt(L, [stream] * n, win, _fmt(E_BF16))
                    assert rc == 0, ccmi.last_error()
                    for a, b in zip(info, finfo):
                        assert list(a.arm_rows) == list(b.arm_rows) and (a.windowed, a.n_grids) == (b.windowed, b.n_grids)
                    grow = need - fneed
                    assert grow % 256 == 0 and 0 <= grow <= 256 * math.ceil(32 * n / 256), (need, fneed)
                    assert _groups(L) == (0, 0)
                assert wins[WARP_CUBIC] == wins[WARP_CUBIC | WARP_CLAMP]


def test_cubic_windows_at_the_corners_and_outside(L, data):
    """Explicit numbers on the 416 x 240 stream at 444: an integer translation reaches one pixel
    further than its crop on every side the frame allows; an output outside the frame plans one
    clamped pixel row / column, as the bilinear window does."""
    d = [data[0]] * 5
    mats = [(1, 0, 0, 0, 1, 0), (1, 0, 408, 0, 1, 232), (1, 0, 100, 0, 1, 50), (1, 0, 5000, 0, 1, 20), (0, 0, -7, 0, 0, 1e6)]
    w, keep = WA._warp(mats, 8, 8, PAD_EDGE | WARP_CUBIC)
    rc, _, _, win, _ = WA._plan(L, d, _fmt(), w, chroma=444)
    assert rc == 0
    # columns floor(x + 0.5 - 0.5) - 2 .. floor(x + 7.5 - 0.5) + 3, clamped
    assert win == [(0, 0, 11, 11), (406, 230, 10, 10), (98, 48, 13, 13), (415, 18, 1, 13), (0, 239, 1, 1)]
    assert win == [R.window(m, 8, 8, 240, 416) for m in mats]
    w, keep = WA._warp(mats, 8, 8, PAD_EDGE)
    rc, _, _, bwin, _ = WA._plan(L, d, _fmt(), w, chroma=444)
    assert bwin[2] == (99, 49, 11, 11)


def test_render_warp_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    mats = [IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20), (-1, 0, 64, 0, 1, 3)]
    with Handle(L, data) as H:
        m = len(index)
        idx, f = (C.c_int * m)(*index), _fmt(E_F16)
        for pad in (0x100, 0x301):
            w, keep = WA._warp(mats, 32, 48, pad, (0.5, 0.5, 0.5))
            geom, info, win, need = (Geom * m)(), (Info * m)(), (Rect * m)(), C.c_size_t(0)
            rc = L.ccmi_latents_render_warp_plan(H.h, idx, m, 0, 0, C.byref(f), C.byref(w), geom, info, win, C.byref(need))
            assert rc == 0, ccmi.last_error()
            rc, gd, _, wind, _ = WA._plan(L, [data[i] for i in index], f, w)
            assert rc == 0, ccmi.last_error()
            assert [(r.x, r.y, r.w, r.h) for r in win] == wind
            assert [_fields(a) for a in geom] == [_fields(b) for b in gd]
        w, keep = WA._warp(mats, 32, 48, 0x200)
        rc = L.ccmi_latents_render_warp_plan(H.h, idx, m, 0, 0, C.byref(f), C.byref(w), geom, None, None, C.byref(need))
        _is_arg_error(rc, 0, "pad")


def test_python_constants():
    from ccmi import decode
    assert (decode.FILTER_TRIANGLE, decode.FILTER_CUBIC, decode.FILTER_CLAMP) == (0, 2, 0x100)
    assert (decode.PAD_FILL, decode.PAD_EDGE, decode.WARP_CUBIC, decode.WARP_CLAMP) == (0, 1, 0x100, 0x200)
    assert decode._interp("bilinear", False) == (0, 0)
    assert decode._interp("bicubic", False) == (2, 0x100)
    assert decode._interp("bicubic", True) == (0x102, 0x300)
    for bad in ("nearest", "Bicubic", "", None):
        with pytest.raises(ValueError, match="interpolation"):
            decode._interp(bad, False)
    with pytest.raises(ValueError, match="clamp"):
        decode._interp("bilinear", True)
