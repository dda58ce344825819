"""ccmi_decode_batch_dev_flt(_plan) / ccmi_latents_render_flt(_plan): the host side of the filtered
formatted output (ccmi_filter).  As tests/test_decode_colour_abi.py: no compute here, the plan calls make
no GPU call (they are header-only), the latent handles are plan-only, and the run entry point is only
ever called with arguments the plan rejects (made-up device pointers that nothing dereferences)."""
import ctypes as C

import pytest

from test_decode_colour_abi import BRIGHTNESS, CONTRAST, _colour
from test_decode_resample_abi import (E_BF16, E_F32, ERR_ARG, FAKE, Geom, Handle, I, Info, P, Rect, Rs, Z, _args, _fields,
                                      _first, _fmt, _is_arg_error, _rects)
from test_decode_warp_abi import IDENT, Warp, _warp

MAX_RADIUS = 15
NAMES = ("ccmi_decode_batch_dev_flt_plan", "ccmi_decode_batch_dev_flt", "ccmi_latents_render_flt_plan",
         "ccmi_latents_render_flt")


class Filter(C.Structure):
    _fields_ = [("radius", C.c_void_p), ("taps", C.c_void_p), ("solarize", C.c_void_p)]


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.ccmi_decode_batch_dev_flt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_flt.argtypes = [P, P, I, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_render_flt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_flt.argtypes = [P, P, I, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for name in NAMES + ("ccmi_decode_batch_dev_col_plan", "ccmi_latents_render_col_plan", "ccmi_latents_decode",
                         "ccmi_decode_last_tail_groups"):
        getattr(lib, name).restype = C.c_int
    return lib


def _filter(frames, solarize=None):
    """frames: per frame the half taps (a list; [] or one tap: radius 0); solarize: None or one threshold
    per frame -> (ccmi_filter, what it points to)"""
    n = len(frames)
    radius = (C.c_int * n)(*[max(len(t) - 1, 0) for t in frames])
    flat = [v for t in frames if len(t) > 1 for v in t]
    taps = (C.c_float * max(len(flat), 1))(*flat)
    th = None if solarize is None else (C.c_float * n)(*solarize)
    return Filter(radius=C.cast(radius, C.c_void_p), taps=C.cast(taps, C.c_void_p),
                  solarize=None if th is None else C.cast(th, C.c_void_p)), (radius, taps, th)


def _ref(x):
    return None if x is None else C.byref(x)


def _plan(lib, data, fmt, flt, colour=None, rects=None, rs=None, warp=None, chroma=444, window=False):
    """(rc, geom, info, windows, workspace bytes) of ccmi_decode_batch_dev_flt_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_flt_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), _ref(warp),
                                            _ref(colour), _ref(flt), geom, info, win if window else None, C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _plan_col(lib, data, fmt, colour=None, rects=None, rs=None, warp=None, chroma=444, window=False):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_col_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), _ref(warp),
                                            _ref(colour), geom, info, win if window else None, C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _run(lib, data, fmt, flt, colour=None, rects=None, rs=None, warp=None, chroma=444):
    """ccmi_decode_batch_dev_flt with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*[FAKE + (i << 32) for i in range(n)])
    cp = (C.c_size_t * n)(*[1 << 30] * n)
    return lib.ccmi_decode_batch_dev_flt(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), _ref(rs), _ref(warp),
                                         _ref(colour), _ref(flt), 0, chroma, None, 0, None)


def _rejected(lib, data, flt, frame, *words, **kw):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned or written"""
    rc, _, _, _, got = _plan(lib, data, _fmt(), flt, **kw)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    kw.pop("window", None)
    _is_arg_error(_run(lib, data, _fmt(), flt, **kw), frame, *words)


def _same_plan(a, b, n):
    for j in range(n):
        assert _fields(a[1][j]) == _fields(b[1][j])
        assert list(a[2][j].arm_rows) == list(b[2][j].arm_rows) and a[2][j].windowed == b[2][j].windowed


def _grow(sizes):
    """the documented formula: per staged frame of oh x ow, 12 oh ow rounded up to 256, + 256"""
    return sum(-(-12 * oh * ow // 256) * 256 + 256 for oh, ow in sizes)


def test_symbols_and_struct_layout(L):
    import ccmi
    from ccmi import decode
    for name in NAMES:
        assert name in ccmi.EXPORTED and name in decode._PROTOS
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(Filter) == 3 * p and Filter.taps.offset == p and Filter.solarize.offset == 2 * p
    assert C.sizeof(decode.Filter) == C.sizeof(Filter) and decode.Filter.solarize.offset == 2 * p
    assert decode.FLT_MAX_RADIUS == MAX_RADIUS


def test_radius_null_or_outside_the_range(L, data):
    import ccmi
    t, keep = _filter([[1.0, 0.0]] * 3)
    norad = Filter(radius=None, taps=t.taps, solarize=None)
    _rejected(L, data, norad, 0, "radii")
    for bad in (-1, 16, 1 << 20):
        f, keep = _filter([[], [0.5, 0.25], []])
        keep[0][2] = bad
        _rejected(L, data, f, 2, "radius", str(bad), "15")
    f, keep = _filter([[0.1] * (MAX_RADIUS + 1)] * 3)  # the largest radius is fine
    rc, *_ = _plan(L, data, _fmt(), f)
    assert rc == 0, ccmi.last_error()


def test_taps_null_while_a_radius_is_set(L, data):
    import ccmi
    f, keep = _filter([[], [0.5, 0.25], []])
    _rejected(L, data, Filter(radius=f.radius, taps=None, solarize=None), 1, "taps", "NULL")
    z, keepz = _filter([[], [], []], [0.5, 2.0, 0.0])  # every radius 0: the taps may be NULL
    rc, *_ = _plan(L, data, _fmt(), Filter(radius=z.radius, taps=None, solarize=z.solarize))
    assert rc == 0, ccmi.last_error()


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), -float("inf")))
def test_non_finite_tap(L, data, bad):
    import ccmi
    for k in (0, 1, 3):
        taps = [0.4, 0.2, 0.05, 0.05]
        taps[k] = bad
        f, keep = _filter([[0.5, 0.25], [], taps])  # the flat array is walked by the frames' own lengths
        _rejected(L, data, f, 2, "tap %d" % k, "finite")
    f, keep = _filter([[-0.5, 2.0, -1e30]] * 3)  # any finite taps are legal
    rc, *_ = _plan(L, data, _fmt(), f)
    assert rc == 0, ccmi.last_error()


def test_nan_threshold(L, data):
    import ccmi
    f, keep = _filter([[], [], []], [0.5, float("nan"), 2.0])
    _rejected(L, data, f, 1, "threshold", "NaN")
    f, keep = _filter([[], [], []], [float("inf"), -float("inf"), -1.0])  # off, always, always
    rc, *_ = _plan(L, data, _fmt(), f)
    assert rc == 0, ccmi.last_error()


def test_errors_on_every_geometry_with_colour_and_from_a_handle(L, data):
    import ccmi
    bad, keep = _filter([[0.5, 0.25], [0.5, float("nan")]])
    good, keepg = _filter([[0.5, 0.25], [0.5, 0.25]])
    w, keepw = _warp([IDENT] * 2, 8, 8)
    _rejected(L, data[:2], bad, 1, "tap 1", rects=[(0, 0, 16, 16)] * 2)
    _rejected(L, data[:2], bad, 1, "tap 1", rects=[(0, 0, 16, 16), (4, 4, 40, 20)], rs=Rs(out_w=8, out_h=8, filter=0))
    _rejected(L, data[:2], bad, 1, "tap 1", warp=w, window=True)
    # everything the _col plan checks stays: a bad colour op (reported first), a bad geometry
    col, keepc = _colour([[(BRIGHTNESS, 1.0)], [(BRIGHTNESS, -2.0)]])
    _rejected(L, data[:2], good, 1, "factor", colour=col)
    _rejected(L, data[:2], good, 0, "output size", rs=Rs(out_w=0, out_h=8, filter=0))
    rs = Rs(out_w=8, out_h=8, filter=0)
    _rejected(L, data[:2], good, 0, "resample", "warp", rs=rs, warp=w)
    with Handle(L, data) as H:
        idx = (C.c_int * 2)(2, 0)
        geom, need = (Geom * 2)(), C.c_size_t(0)
        f = _fmt()
        rc = L.ccmi_latents_render_flt_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, None, C.byref(bad), geom, None,
                                            None, C.byref(need))
        _is_arg_error(rc, 1, "tap 1")
        assert need.value == 0
        op, cp = (C.c_void_p * 2)(FAKE, FAKE), (C.c_size_t * 2)(1 << 30, 1 << 30)
        rc = L.ccmi_latents_render_flt(H.h, idx, 2, None, op, cp, C.byref(f), None, None, None, C.byref(good), 0, 444, None, 0,
                                       None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


def test_null_arguments(L, data):
    keep, sp, ln = _args(data)
    geom, need, win = (Geom * 3)(), C.c_size_t(0), (Rect * 3)()
    f = _fmt()
    flt, keepf = _filter([[0.5, 0.25]] * 3)
    nomat = Warp(out_w=8, out_h=8, pad=0, matrix=None)
    plan = L.ccmi_decode_batch_dev_flt_plan
    for args in ((sp, ln, 3, None, 0, 444, None, None, None, None, C.byref(flt), geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, C.byref(nomat), None, C.byref(flt), geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(flt), None, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(flt), geom, None, win, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(flt), geom, None, None, None)):
        _is_arg_error(plan(*args), 0, "null")
    # a call that only plans reports no launches
    a, b = C.c_int(7), C.c_int(7)
    assert plan(sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(flt), geom, None, None, C.byref(need)) == 0
    assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def test_null_filter_and_no_staged_frame_plan_like_col(L, data):
    """filter NULL, and a filter under which no frame takes the stage (every radius 0, thresholds above 1 or
    none): geometry, info, windows and workspace of the _col plan, to the byte -- with and without colour
    ops, on every geometry."""
    import ccmi
    n = 3
    rects = [(16, 8, 64, 48), (100, 200, 300, 100), (0, 0, 32, 32)]
    none, keep0 = _filter([[], [], []])
    off, keep1 = _filter([[], [1.0], []], [2.0, 1.0000001, float("inf")])  # a centre tap alone is radius 0
    col, keepc = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8)]])
    f = _fmt(E_BF16)
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    cases = (dict(rects=None), dict(rects=[(16, 8, 64, 48)] * n), dict(rects=rects, rs=Rs(32, 24, 0)),
             dict(warp=w, window=True))
    for kw in cases:
        for c in (None, col):
            base = _plan_col(L, data, f, c, **kw)
            assert base[0] == 0, ccmi.last_error()
            for flt in (None, none, off):
                got = _plan(L, data, f, flt, c, **kw)
                assert got[0] == 0, ccmi.last_error()
                _same_plan(got, base, n)
                assert got[3] == base[3] and got[4] == base[4]


def test_workspace_grows_by_the_documented_formula(L, data):
    """Mixed batches: per frame that takes the stage one float32 frame [3][oh][ow] rounded up to 256 bytes and
    256 bytes of tables; the others add nothing; radii and thresholds do not change it."""
    import ccmi
    n = 3
    t3, t15 = [0.4, 0.2, 0.1], [0.1] * 16
    f = _fmt(E_BF16)
    col, keepc = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8)]])
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    frame = [(240, 416), (720, 1280), (768, 512)]  # (h, w) of the three streams
    rects = [(16, 8, 65, 47), (100, 200, 301, 99), (0, 0, 33, 31)]
    region = [(r[3], r[2]) for r in rects]
    geoms = ((dict(rects=None), frame), (dict(rects=rects), region), (dict(rects=rects, rs=Rs(33, 21, 0)), [(21, 33)] * n),
             (dict(warp=w, window=True), [(16, 24)] * n))
    filters = (([t3, [], []], None, (0,)), ([[], t15, t3], None, (1, 2)), ([t3, t15, t3], [0.5, 2.0, 0.0], (0, 1, 2)),
               ([[], [], []], [2.0, 0.5, 1.0], (1, 2)), ([[], [], t15], [0.0, 2.0, 2.0], (0, 2)))
    for kw, sizes in geoms:
        for c in (None, col):
            base = _plan_col(L, data, f, c, **kw)
            assert base[0] == 0, ccmi.last_error()
            for taps, th, staged in filters:
                flt, keep = _filter(taps, th)
                got = _plan(L, data, f, flt, c, **kw)
                assert got[0] == 0, ccmi.last_error()
                _same_plan(got, base, n)
                assert got[3] == base[3]
                assert got[4] - base[4] == _grow([sizes[j] for j in staged]), (kw, taps, th)
    assert frame == [(g.height, g.width) for g in _plan_col(L, data, f)[1]]


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    m = len(index)
    rects = [(0, 0, 64, 48), (640, 360, 200, 100), (16, 8, 100, 60), (3, 5, 40, 40)]
    flt, keep = _filter([[0.5, 0.25], [], [], [0.2] * 12], [2.0, 2.0, 0.5, 0.5])
    f = _fmt(E_F32)
    rs = Rs(32, 24, 0)
    with Handle(L, data) as H:
        idx = (C.c_int * m)(*index)
        geom, info, need = (Geom * m)(), (Info * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_flt_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                            C.byref(flt), geom, info, None, C.byref(need))
        assert rc == 0, ccmi.last_error()
        got = _plan(L, [data[i] for i in index], f, flt, rects=rects, rs=rs)
        assert got[0] == 0, ccmi.last_error()
        for a, b in zip(geom, got[1]):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (32, 24)
        n0 = C.c_size_t(0)
        assert L.ccmi_latents_render_col_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              geom, None, None, C.byref(n0)) == 0
        assert need.value - n0.value == _grow([(24, 32)] * 3)
        n1 = C.c_size_t(0)
        assert L.ccmi_latents_render_flt_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              None, geom, None, None, C.byref(n1)) == 0
        assert n1.value == n0.value
