"""ccmi_decode_batch_dev_warp(_plan) / ccmi_latents_render_warp(_plan): the host side of the
warped formatted output (ccmi_warp).  As tests/test_decode_resample_abi.py: no compute here, the
plan calls make no GPU call, the latent handles are plan-only, and the run entry point is only
ever called with arguments the plan rejects (made-up device pointers that nothing dereferences)."""
import ctypes as C
import math

import numpy as np
import pytest

import warp_ref as W
from test_decode_resample_abi import (E_BF16, E_F16, E_F32, ERR_ARG, FAKE, Fmt, Geom, Handle, I, Info, P, Rect, Z, _args,
                                      _fields, _first, _fmt, _header_only, _is_arg_error, _rects)

PAD_FILL, PAD_EDGE = 0, 1
IDENT = (1, 0, 0, 0, 1, 0)


class Warp(C.Structure):
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("pad", C.c_int), ("fill", C.c_float * 3), ("matrix", C.c_void_p)]


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    lib.ccmi_decode_batch_dev_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_decode_batch_dev_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_warp.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_latents_render_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_latents_render_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_latents_render_warp.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for f in (lib.ccmi_decode_batch_dev_fmt_plan, lib.ccmi_decode_batch_dev_warp_plan, lib.ccmi_decode_batch_dev_warp,
              lib.ccmi_latents_decode, lib.ccmi_latents_render_fmt_plan, lib.ccmi_latents_render_warp_plan,
              lib.ccmi_latents_render_warp, lib.ccmi_decode_last_tail_groups):
        f.restype = C.c_int
    return lib


def _warp(mats, ow, oh, pad=PAD_FILL, fill=(0.0, 0.0, 0.0)):
    """(ccmi_warp, the matrix array it points to)"""
    a = np.ascontiguousarray(np.asarray(mats, dtype=np.float32).reshape(-1, 6))
    w = Warp(out_w=ow, out_h=oh, pad=pad, matrix=a.ctypes.data)
    for c in range(3):
        w.fill[c] = fill[c]
    return w, a


def _plan(lib, data, fmt, warp, bitdepth=0, chroma=0):
    """(rc, geom, info, windows, workspace bytes) of ccmi_decode_batch_dev_warp_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_warp_plan(sp, ln, n, bitdepth, chroma, C.byref(fmt), C.byref(warp), geom, info, win,
                                             C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _plan_fmt(lib, data, rects, fmt, bitdepth=0, chroma=0):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_fmt_plan(sp, ln, n, _rects(rects, n), bitdepth, chroma, C.byref(fmt), geom, info,
                                            C.byref(need))
    return rc, geom, info, need.value


def _run(lib, data, fmt, warp, caps, chroma=0):
    """ccmi_decode_batch_dev_warp with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*[FAKE + (i << 32) for i in range(n)])
    cp = (C.c_size_t * n)(*caps)
    return lib.ccmi_decode_batch_dev_warp(sp, ln, n, op, cp, C.byref(fmt), C.byref(warp), 0, chroma, None, 0, None)


def _rejected(lib, data, mats, ow, oh, frame, *words, pad=PAD_FILL, fill=(0.0, 0.0, 0.0), chroma=444):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned"""
    w, keep = _warp(mats, ow, oh, pad, fill)
    rc, _, _, _, got = _plan(lib, data, _fmt(), w, chroma=chroma)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    rc = _run(lib, data, _fmt(), w, [1 << 30] * len(data), chroma=chroma)
    _is_arg_error(rc, frame, *words)


@pytest.mark.parametrize("ow,oh", ((0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385), (1 << 30, 1 << 30)))
def test_output_size_outside_the_range(L, data, ow, oh):
    _rejected(L, data[:2], [IDENT] * 2, ow, oh, 0, "output size", "16384")


def test_output_size_at_the_limits_is_accepted(L, data):
    import ccmi
    for ow, oh in ((1, 1), (16384, 1), (1, 16384)):
        w, keep = _warp([IDENT], ow, oh)
        rc, geom, _, win, _ = _plan(L, data[:1], _fmt(), w, chroma=444)
        assert rc == 0, ccmi.last_error()
        assert (geom[0].width, geom[0].height, geom[0].elems) == (ow, oh, 3 * ow * oh)


def test_unknown_pad(L, data):
    for pad in (2, -1, 77):
        _rejected(L, data[:2], [IDENT] * 2, 8, 8, 0, "pad", pad=pad)


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), -float("inf")))
def test_non_finite_matrix_entry_or_fill(L, data, bad):
    for k in range(6):
        m = list(IDENT)
        m[k] = bad
        _rejected(L, data, [IDENT, m, IDENT], 8, 8, 1, "matrix", "finite")
    for c in range(3):
        fill = [0.0, 0.0, 0.0]
        fill[c] = bad
        for pad in (PAD_FILL, PAD_EDGE):
            _rejected(L, data, [IDENT] * 3, 8, 8, 0, "fill", "finite", pad=pad, fill=fill)


def test_the_reach_bound(L, data):
    """|m0| out_w + |m1| out_h + |m2| <= 2^22 per row: at the bound accepted, one float32 step above refused."""
    import ccmi
    top = 2.0 ** 22
    over = float(np.nextafter(np.float32(top), np.float32(np.inf)))
    for row in (0, 1):
        def mat(a, b, c):
            m = list(IDENT)
            m[3 * row: 3 * row + 3] = [a, b, c]
            return m
        ok = (mat(0, 0, top), mat(0, 0, -top), mat(top / 16, 0, 0), mat(-1, 1, top - 32), mat(0, -top / 16, 0))
        for m in ok:
            w, keep = _warp([IDENT, m], 16, 16, PAD_EDGE)
            rc, *_ = _plan(L, data[:2], _fmt(), w, chroma=444)
            assert rc == 0, (m, ccmi.last_error())
        for m in (mat(0, 0, over), mat(0, 0, -over), mat(over / 16, 0, 0), mat(1, -1, top - 31), mat(1e30, 0, 0),
                  mat(0, -3e38, 3e38)):
            _rejected(L, data[:2], [IDENT, m], 16, 16, 1, "2^22")


def test_420_needs_an_even_frame(L):
    import ccmi
    for h, w in ((63, 64), (64, 63), (21, 37)):
        odd = [_header_only(64, 64), _header_only(h, w)]
        _rejected(L, odd, [IDENT] * 2, 8, 8, 1, "even", "444", chroma=0)
        _rejected(L, odd, [IDENT] * 2, 8, 8, 1, "even", chroma=420)
        wp, keep = _warp([IDENT] * 2, 8, 8)
        rc, geom, *_ = _plan(L, odd, _fmt(), wp, chroma=444)
        assert rc == 0, ccmi.last_error()
        assert geom[1].chroma == 444


def test_null_arguments_and_the_group_counters(L, data):
    import ccmi
    keep, sp, ln = _args(data)
    geom, need = (Geom * 3)(), C.c_size_t(0)
    f = _fmt()
    w, keep_w = _warp([IDENT] * 3, 8, 8)
    nomat = Warp(out_w=8, out_h=8, pad=0, matrix=None)
    plan = L.ccmi_decode_batch_dev_warp_plan
    for args in ((sp, ln, 3, 0, 444, None, C.byref(w), geom, None, None, C.byref(need)),
                 (sp, ln, 3, 0, 444, C.byref(f), None, geom, None, None, C.byref(need)),
                 (sp, ln, 3, 0, 444, C.byref(f), C.byref(nomat), geom, None, None, C.byref(need)),
                 (sp, ln, 3, 0, 444, C.byref(f), C.byref(w), None, None, None, C.byref(need)),
                 (sp, ln, 3, 0, 444, C.byref(f), C.byref(w), geom, None, None, None)):
        _is_arg_error(plan(*args), 0, "null")
    op, cp = (C.c_void_p * 3)(*[FAKE] * 3), (C.c_size_t * 3)(*[1 << 30] * 3)
    run = L.ccmi_decode_batch_dev_warp
    _is_arg_error(run(sp, ln, 3, op, cp, C.byref(f), None, 0, 444, None, 0, None), 0, "null")
    _is_arg_error(run(sp, ln, 3, op, cp, C.byref(f), C.byref(nomat), 0, 444, None, 0, None), 0, "null")
    _is_arg_error(run(sp, ln, 3, None, cp, C.byref(f), C.byref(w), 0, 444, None, 0, None), 0, "null")
    with Handle(L, data) as H:
        _is_arg_error(L.ccmi_latents_render_warp_plan(H.h, None, 3, 0, 444, C.byref(f), C.byref(nomat), geom, None, None,
                                                      C.byref(need)), 0, "null")
        rc = L.ccmi_latents_render_warp(H.h, None, 3, op, cp, C.byref(f), C.byref(w), 0, 444, None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()
    # a call that only plans reports no launches; window and info are optional
    a, b = C.c_int(7), C.c_int(7)
    assert plan(sp, ln, 3, 0, 444, C.byref(f), C.byref(w), geom, None, None, C.byref(need)) == 0, ccmi.last_error()
    assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def _random_matrices(rng, n, H, W_, oh, ow):
    from test_decode_warp_ref import random_matrix
    return [random_matrix(rng, H, W_, oh, ow) for _ in range(n)]


SIZES = ((240, 416), (720, 1280), None)  # the third: the Kodak stream's own


def test_windows_hold_every_tap_and_size_the_workspace(L, data):
    """200 random matrices per stream: the window is the rule of warp_ref.window() -- a superset of
    the float32 contract's in-frame taps, never empty, inside the frame, even at 420 -- the
    geometry is the output's, and the workspace is the _fmt plan's for roi = window but for the
    argument table, whose entry is 32 bytes longer per frame (the matrix, the window's origin and
    the frame size), rounded to 256 for the call."""
    import ccmi
    rng = np.random.default_rng(77)
    ident = _warp([IDENT], 8, 8)
    for i, stream in enumerate(data):
        g0 = _plan(L, [stream], _fmt(), ident[0])[1][0]
        H, W_, chroma = ccmi_frame(L, stream)
        assert chroma == (420 if i < 2 else 444) and g0.chroma == chroma
        for oh, ow in ((224, 224), (17, 39), (1, 1), (8, 300)):
            n = 50
            mats = _random_matrices(rng, n, H, W_, oh, ow)
            for pad in (PAD_FILL, PAD_EDGE):
                w, keep = _warp(mats, ow, oh, pad, (0.1, 0.2, 0.3))
                rc, geom, info, win, need = _plan(L, [stream] * n, _fmt(E_BF16), w)
                assert rc == 0, ccmi.last_error()
                for j, m in enumerate(mats):
                    x, y, ww, hh = win[j]
                    assert win[j] == W.window(m, oh, ow, H, W_, even=chroma == 420), (i, j)
                    assert ww >= 1 and hh >= 1 and x >= 0 and y >= 0 and x + ww <= W_ and y + hh <= H
                    if chroma == 420:
                        assert (x | y | ww | hh) & 1 == 0
                    ty, tx = W.taps_in_frame(m, oh, ow, H, W_)
                    assert not ((tx < x) | (tx >= x + ww) | (ty < y) | (ty >= y + hh)).any(), (i, j)
                    g = geom[j]
                    assert (g.width, g.height, g.elems) == (ow, oh, 3 * ow * oh)
                    assert (g.bitdepth, g.chroma, g.frame_data_type) == (g0.bitdepth, g0.chroma, g0.frame_data_type)
                rc, _, finfo, fneed = _plan_fmt(L, [stream] * n, win, _fmt(E_BF16))
                assert rc == 0, ccmi.last_error()
                for a, b in zip(info, finfo):
                    assert list(a.arm_rows) == list(b.arm_rows) and (a.windowed, a.n_grids) == (b.windowed, b.n_grids)
                grow = need - fneed
                assert grow % 256 == 0 and 0 <= grow <= 256 * math.ceil(32 * n / 256), (need, fneed)


def ccmi_frame(lib, stream):
    """(H, W, chroma of its own samples) of a stream, from the identity plan at chroma 0"""
    w, keep = _warp([IDENT], 1, 1)
    h, wd = int.from_bytes(stream[2:4], "big"), int.from_bytes(stream[4:6], "big")
    rc, geom, *_ = _plan(lib, [stream], _fmt(), w)
    assert rc == 0
    return h, wd, geom[0].chroma


def test_identity_at_frame_size_is_the_whole_frame(L, data):
    """m = identity, out = the frame: the window is the frame, and so are the info and (but for the
    table) the workspace of the whole-frame _fmt plan."""
    import ccmi
    for stream in data:
        H, W_, _ = ccmi_frame(L, stream)
        w, keep = _warp([IDENT], W_, H)
        rc, geom, info, win, need = _plan(L, [stream], _fmt(), w)
        assert rc == 0, ccmi.last_error()
        assert win == [(0, 0, W_, H)] and (geom[0].width, geom[0].height) == (W_, H)
        rc, _, finfo, fneed = _plan_fmt(L, [stream], None, _fmt())
        assert rc == 0
        assert list(info[0].arm_rows) == list(finfo[0].arm_rows)
        assert 0 <= need - fneed <= 256 and (need - fneed) % 256 == 0


def test_outside_and_singular_matrices_plan_a_clamped_window(L, data):
    import ccmi
    d = [data[0]] * 4  # 416 x 240, 420
    mats = [(1, 0, 5000, 0, 1, 20), (1, 0, 20, 0, 1, -5000), (0, 0, 100.25, 0, 0, 50.75), (0, 0, -7, 0, 0, 1e6)]
    w, keep = _warp(mats, 16, 24, PAD_EDGE)
    rc, geom, info, win, need = _plan(L, d, _fmt(), w)
    assert rc == 0, ccmi.last_error()
    assert win == [(414, 18, 2, 28), (18, 0, 20, 2), (98, 48, 4, 6), (0, 238, 2, 2)]
    assert win == [W.window(m, 24, 16, 240, 416, even=True) for m in mats]
    rc, geom, info, win, need = _plan(L, d, _fmt(), w, chroma=444)
    assert win == [(415, 19, 1, 27), (19, 0, 19, 1), (98, 49, 4, 4), (0, 239, 1, 1)]


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    mats = [IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20), (-1, 0, 64, 0, 1, 3)]
    with Handle(L, data) as H:
        m = len(index)
        idx = (C.c_int * m)(*index)
        f = _fmt(E_F16)
        w, keep = _warp(mats, 32, 48, PAD_FILL, (0.5, 0.5, 0.5))
        geom, info, win, need = (Geom * m)(), (Info * m)(), (Rect * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_warp_plan(H.h, idx, m, 0, 0, C.byref(f), C.byref(w), geom, info, win, C.byref(need))
        assert rc == 0, ccmi.last_error()
        rc, gd, idd, wind, _ = _plan(L, [data[i] for i in index], f, w)
        assert rc == 0, ccmi.last_error()
        assert [(r.x, r.y, r.w, r.h) for r in win] == wind
        for a, b in zip(geom, gd):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (32, 48)
        # the render workspace: the _fmt render plan's with roi = window, but for the table
        g2, n2 = (Geom * m)(), C.c_size_t(0)
        assert L.ccmi_latents_render_fmt_plan(H.h, idx, m, win, 0, 0, C.byref(f), g2, None, C.byref(n2)) == 0
        assert 0 <= need.value - n2.value <= 256 and (need.value - n2.value) % 256 == 0
        # errors name the output frame
        bad, keepb = _warp(mats[:2] + [(float("nan"),) * 6] + mats[3:], 32, 48)
        rc = L.ccmi_latents_render_warp_plan(H.h, idx, m, 0, 0, C.byref(f), C.byref(bad), geom, None, None, C.byref(need))
        _is_arg_error(rc, 2, "finite")
        idx_bad = (C.c_int * m)(1, 1, 3, 2)
        rc = L.ccmi_latents_render_warp_plan(H.h, idx_bad, m, 0, 0, C.byref(f), C.byref(w), geom, None, None, C.byref(need))
        _is_arg_error(rc, 2, "index")


def test_capacity_and_aliasing_use_the_output_size(L, data):
    d = [data[0], data[0]]
    ow, oh = 10, 6
    w, keep = _warp([IDENT, (2, 0, 16, 0, 2, 8)], ow, oh)
    for elem, size in ((E_F32, 4), (E_F16, 2)):
        for strides in ((0, 0, 0), (1, 3 * ow, 3), (40 * 80, 80, 1)):
            sc, sy, sx = strides if any(strides) else (ow * oh, ow, 1)
            need = (2 * sc + (oh - 1) * sy + (ow - 1) * sx + 1) * size
            f = _fmt(elem, strides)
            _is_arg_error(_run(L, d, f, w, [need, need - 1]), 1, str(need), str(need - 1))
            _is_arg_error(_run(L, d, f, w, [need - size, need]), 0, str(need))
    rc, *_ = _plan(L, d, _fmt(strides=(32, 8, 1)), w)
    _is_arg_error(rc, 0, "alias")


def test_affine_matrix_helper():
    """decode.affine_matrix against explicit numbers: angle = pi / 2, scale = 2 and flip."""
    from ccmi import decode
    size, centre = (6, 8), (20.0, 10.0)  # out_h 6, out_w 8
    a = decode.affine_matrix(size, centre)
    assert a.dtype == np.float32 and a.shape == (2, 3)
    assert a.tolist() == [[1, 0, 16], [0, 1, 7]]  # the crop at (16, 7): centre - out / 2
    # angle pi / 2: xs = cx - dy, ys = cy + dx; at k = 0, i = 0: dx = -3.5, dy = -2.5
    r = decode.affine_matrix(size, centre, angle=math.pi / 2)
    assert np.allclose(r, [[0, -1, 20 + 3], [1, 0, 10 - 4]], atol=1e-6, rtol=0)
    assert np.allclose(r @ [0.5, 0.5, 1], [20 + 2.5, 10 - 3.5], atol=1e-5)
    # scale 2: half as many frame pixels a side, about the same centre
    s = decode.affine_matrix(size, centre, scale=2.0)
    assert s.tolist() == [[0.5, 0, 18], [0, 0.5, 8.5]]
    # flip: dx negated
    f = decode.affine_matrix(size, centre, flip=True)
    assert f.tolist() == [[-1, 0, 24], [0, 1, 7]]
    both = decode.affine_matrix(size, centre, angle=math.pi / 2, scale=2.0, flip=True)
    assert np.allclose(both, [[0, -0.5, 21.5], [-0.5, 0, 12]], atol=1e-6, rtol=0)
