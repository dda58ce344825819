"""ccmi_decode_batch_dev_col(_plan) / ccmi_latents_render_col(_plan): the host side of the
coloured formatted output (ccmi_colour).  As tests/test_decode_warp_abi.py: no compute here, the
plan calls make no GPU call (they are header-only), the latent handles are plan-only, and the run
entry point is only ever called with arguments the plan rejects (made-up device pointers that
nothing dereferences)."""
import ctypes as C

import pytest

from test_decode_resample_abi import (E_BF16, E_F32, ERR_ARG, FAKE, Geom, Handle, I, Info, P, Rect, Rs, Z, _args, _fields,
                                      _first, _fmt, _is_arg_error, _rects)
from test_decode_warp_abi import IDENT, Warp, _warp

BRIGHTNESS, SATURATION, CONTRAST, MATRIX = 0, 1, 2, 3
MAX_OPS = 8
EYE = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


class Op(C.Structure):
    _fields_ = [("op", C.c_int), ("v", C.c_float * 12)]


class Colour(C.Structure):
    _fields_ = [("count", C.c_void_p), ("ops", C.c_void_p)]


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    lib.ccmi_decode_batch_dev_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_col.argtypes = [P, P, I, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_render_col_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_col.argtypes = [P, P, I, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_warp_plan.argtypes = [P, P, I, I, I, P, P, P, P, P, P]
    lib.ccmi_latents_render_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for f in (lib.ccmi_decode_batch_dev_col_plan, lib.ccmi_decode_batch_dev_col, lib.ccmi_latents_render_col_plan,
              lib.ccmi_latents_render_col, lib.ccmi_decode_batch_dev_rs_plan, lib.ccmi_decode_batch_dev_warp_plan,
              lib.ccmi_latents_render_rs_plan, lib.ccmi_latents_decode, lib.ccmi_decode_last_tail_groups):
        f.restype = C.c_int
    return lib


def _colour(frames):
    """frames: per frame a list of (op, values) -> (ccmi_colour, what it points to)"""
    counts = (C.c_int * len(frames))(*[len(f) for f in frames])
    flat = (Op * max(sum(counts), 1))()
    k = 0
    for f in frames:
        for op, v in f:
            flat[k].op = op
            v = v if hasattr(v, "__len__") else (v,)
            for e, x in enumerate(v):
                flat[k].v[e] = x
            k += 1
    return Colour(count=C.cast(counts, C.c_void_p), ops=C.cast(flat, C.c_void_p)), (counts, flat)


def _ref(x):
    return None if x is None else C.byref(x)


def _plan(lib, data, fmt, colour, rects=None, rs=None, warp=None, chroma=444, window=False):
    """(rc, geom, info, windows, workspace bytes) of ccmi_decode_batch_dev_col_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_col_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), _ref(warp),
                                            _ref(colour), geom, info, win if window else None, C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _run(lib, data, fmt, colour, rects=None, rs=None, warp=None, chroma=444):
    """ccmi_decode_batch_dev_col with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*[FAKE + (i << 32) for i in range(n)])
    cp = (C.c_size_t * n)(*[1 << 30] * n)
    return lib.ccmi_decode_batch_dev_col(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), _ref(rs), _ref(warp),
                                         _ref(colour), 0, chroma, None, 0, None)


def _rejected(lib, data, frames, frame, *words, **kw):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned"""
    col, keep = _colour(frames)
    rc, _, _, _, got = _plan(lib, data, _fmt(), col, **kw)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    kw.pop("window", None)
    _is_arg_error(_run(lib, data, _fmt(), col, **kw), frame, *words)


def test_struct_layout():
    """ccmi_colour_op: an int and 12 floats, 52 bytes; ccmi_colour: two pointers"""
    assert C.sizeof(Op) == 52 and Op.v.offset == 4 and C.alignment(Op) == 4
    assert C.sizeof(Colour) == 2 * C.sizeof(C.c_void_p) and Colour.ops.offset == C.sizeof(C.c_void_p)
    from ccmi import decode
    assert C.sizeof(decode.ColourOp) == 52 and decode.ColourOp.v.offset == 4
    assert C.sizeof(decode.Colour) == C.sizeof(Colour) and decode.Colour.ops.offset == Colour.ops.offset
    assert (decode.COL_BRIGHTNESS, decode.COL_SATURATION, decode.COL_CONTRAST, decode.COL_MATRIX) == (0, 1, 2, 3)
    assert decode.COL_MAX_OPS == MAX_OPS


def test_rs_and_warp_both_given(L, data):
    col, keep = _colour([[(BRIGHTNESS, 1.5)]] * 2)
    w, keepw = _warp([IDENT] * 2, 8, 8)
    rs = Rs(out_w=8, out_h=8, filter=0)
    for c in (col, None):
        rc, *_, got = _plan(L, data[:2], _fmt(), c, rs=rs, warp=w)
        _is_arg_error(rc, 0, "resample", "warp")
        assert got == 0
        _is_arg_error(_run(L, data[:2], _fmt(), c, rs=rs, warp=w), 0, "resample", "warp")
    # a warp takes no roi
    rc, *_ = _plan(L, data[:2], _fmt(), col, rects=[(0, 0, 8, 8)] * 2, warp=w)
    _is_arg_error(rc, 0, "roi")


def test_unknown_op(L, data):
    for op in (4, -1, 77):
        _rejected(L, data, [[], [(BRIGHTNESS, 1.0), (op, 1.0)], []], 1, "unknown op", str(op))


def test_more_than_8_ops(L, data):
    import ccmi
    _rejected(L, data, [[(BRIGHTNESS, 1.0)], [], [(SATURATION, 1.1)] * (MAX_OPS + 1)], 2, "9 colour ops", "8")
    col, keep = _colour([[(SATURATION, 1.1)] * MAX_OPS] * 3)
    rc, *_ = _plan(L, data, _fmt(), col)
    assert rc == 0, ccmi.last_error()
    # a negative count
    col, keep = _colour([[], [], []])
    keep[0][1] = -1
    rc, *_ = _plan(L, data, _fmt(), col)
    _is_arg_error(rc, 1, "-1 colour ops")


def test_two_contrast_ops_in_one_frame(L, data):
    import ccmi
    _rejected(L, data, [[(CONTRAST, 1.2)], [(CONTRAST, 1.2), (BRIGHTNESS, 1.0), (CONTRAST, 0.5)], []], 1, "contrast", "0 and 2")
    col, keep = _colour([[(CONTRAST, 1.2)]] * 3)  # one per frame in every frame is fine
    rc, *_ = _plan(L, data, _fmt(), col)
    assert rc == 0, ccmi.last_error()


@pytest.mark.parametrize("bad", (-0.5, -1e-30, float("nan"), float("inf"), -float("inf")))
def test_negative_or_non_finite_factor(L, data, bad):
    for op in (BRIGHTNESS, SATURATION, CONTRAST):
        _rejected(L, data, [[(BRIGHTNESS, 0.0)], [(MATRIX, EYE)], [(MATRIX, EYE), (op, bad)]], 2, "op 1", "factor")


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), -float("inf")))
def test_non_finite_matrix_entry(L, data, bad):
    import ccmi
    for e in range(12):
        m = list(EYE)
        m[e] = bad
        _rejected(L, data, [[(MATRIX, m)], [], []], 0, "matrix entry %d" % e, "finite")
    # negative entries are what an inversion is made of
    col, keep = _colour([[(MATRIX, (-1, 0, 0, 1, 0, -1, 0, 1, 0, 0, -1, 1))]] * 3)
    rc, *_ = _plan(L, data, _fmt(), col)
    assert rc == 0, ccmi.last_error()


def test_errors_on_every_geometry_and_from_a_handle(L, data):
    bad = [[(BRIGHTNESS, 1.0)], [(BRIGHTNESS, -2.0)]]
    w, keepw = _warp([IDENT] * 2, 8, 8)
    _rejected(L, data[:2], bad, 1, "factor", rects=[(0, 0, 16, 16)] * 2)
    _rejected(L, data[:2], bad, 1, "factor", rects=[(0, 0, 16, 16), (4, 4, 40, 20)], rs=Rs(out_w=8, out_h=8, filter=0))
    _rejected(L, data[:2], bad, 1, "factor", warp=w, window=True)
    # the geometry's own checks stay: an output size outside the range, a non-finite warp matrix
    col, keep = _colour([[(BRIGHTNESS, 1.0)]] * 2)
    rc, *_ = _plan(L, data[:2], _fmt(), col, rs=Rs(out_w=0, out_h=8, filter=0))
    _is_arg_error(rc, 0, "output size")
    nanw, keepn = _warp([IDENT, (float("nan"),) * 6], 8, 8)
    rc, *_ = _plan(L, data[:2], _fmt(), col, warp=nanw)
    _is_arg_error(rc, 1, "finite")
    with Handle(L, data) as H:
        idx = (C.c_int * 2)(2, 0)
        geom, need = (Geom * 2)(), C.c_size_t(0)
        bcol, keepb = _colour(bad)
        f = _fmt()
        rc = L.ccmi_latents_render_col_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, C.byref(bcol), geom, None,
                                            None, C.byref(need))
        _is_arg_error(rc, 1, "factor")
        op, cp = (C.c_void_p * 2)(FAKE, FAKE), (C.c_size_t * 2)(1 << 30, 1 << 30)
        import ccmi
        rc = L.ccmi_latents_render_col(H.h, idx, 2, None, op, cp, C.byref(f), None, None, C.byref(col), 0, 444, None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


def test_null_arguments(L, data):
    keep, sp, ln = _args(data)
    geom, need, win = (Geom * 3)(), C.c_size_t(0), (Rect * 3)()
    f = _fmt()
    col, keepc = _colour([[(BRIGHTNESS, 1.0)]] * 3)
    nomat = Warp(out_w=8, out_h=8, pad=0, matrix=None)
    plan = L.ccmi_decode_batch_dev_col_plan
    for args in ((sp, ln, 3, None, 0, 444, None, None, None, C.byref(col), geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, C.byref(nomat), C.byref(col), geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, C.byref(col), None, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, C.byref(col), geom, None, win, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, C.byref(col), geom, None, None, None)):
        _is_arg_error(plan(*args), 0, "null")
    nocount = Colour(count=None, ops=C.cast(keepc[1], C.c_void_p))
    _is_arg_error(plan(sp, ln, 3, None, 0, 444, C.byref(f), None, None, C.byref(nocount), geom, None, None, C.byref(need)),
                  0, "counts")
    noops = Colour(count=C.cast(keepc[0], C.c_void_p), ops=None)
    _is_arg_error(plan(sp, ln, 3, None, 0, 444, C.byref(f), None, None, C.byref(noops), geom, None, None, C.byref(need)),
                  0, "NULL")
    # a call that only plans reports no launches
    a, b = C.c_int(7), C.c_int(7)
    assert plan(sp, ln, 3, None, 0, 444, C.byref(f), None, None, C.byref(col), geom, None, None, C.byref(need)) == 0
    assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def _plan_rs(lib, data, rects, fmt, rs, chroma=444):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_rs_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), geom, info,
                                           C.byref(need))
    return rc, geom, info, need.value


def _plan_warp(lib, data, fmt, warp, chroma=444):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_warp_plan(sp, ln, n, 0, chroma, C.byref(fmt), C.byref(warp), geom, info, win, C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _same_plan(a, b, n):
    for j in range(n):
        assert _fields(a[1][j]) == _fields(b[1][j])
        assert list(a[2][j].arm_rows) == list(b[2][j].arm_rows) and a[2][j].windowed == b[2][j].windowed


def test_null_colour_and_zero_counts_plan_like_rs_and_warp(L, data):
    """colour NULL, and a colour whose every count is 0: geometry, info, windows and workspace of
    the _rs / _warp plan, byte for byte; ops grow the workspace by the op tables and the
    accumulators, and by nothing that depends on which ops they are."""
    import ccmi
    n = 3
    rects = [(16, 8, 64, 48), (100, 200, 300, 100), (0, 0, 32, 32)]
    zero, keepz = _colour([[]] * n)
    some, keeps = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8), (MATRIX, EYE)]])
    full, keepf = _colour([[(CONTRAST, 0.8)] + [(MATRIX, EYE)] * 7] * n)
    f = _fmt(E_BF16)
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    cases = (dict(rects=None, rs=None), dict(rects=[(16, 8, 64, 48)] * n, rs=None), dict(rects=rects, rs=Rs(32, 24, 0)))
    for kw in cases:
        base = _plan_rs(L, data, kw["rects"], f, kw["rs"])
        assert base[0] == 0, ccmi.last_error()
        for col in (None, zero):
            got = _plan(L, data, f, col, **kw)
            assert got[0] == 0, ccmi.last_error()
            _same_plan(got, base, n)
            assert got[4] == base[3]
        grown = [_plan(L, data, f, col, **kw) for col in (some, full)]
        for g in grown:
            assert g[0] == 0, ccmi.last_error()
            _same_plan(g, base, n)
        # per frame: an op table of 8 + 8 + 8 x 52 = 432 bytes; per call: 8 bytes per frame rounded to 256
        assert grown[0][4] == grown[1][4]
        grow = grown[0][4] - base[3]
        assert grow % 256 == 0 and 256 < grow <= 256 * (-(-432 * n // 256) + 1), grow
    base = _plan_warp(L, data, f, w)
    assert base[0] == 0, ccmi.last_error()
    for col in (None, zero):
        got = _plan(L, data, f, col, warp=w, window=True)
        assert got[0] == 0, ccmi.last_error()
        _same_plan(got, base, n)
        assert got[3] == base[3] and got[4] == base[4]
    got = _plan(L, data, f, some, warp=w, window=True)
    assert got[0] == 0 and got[3] == base[3]
    assert 256 < got[4] - base[4] <= 256 * (-(-432 * n // 256) + 1)


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    m = len(index)
    rects = [(0, 0, 64, 48), (640, 360, 200, 100), (16, 8, 100, 60), (3, 5, 40, 40)]
    col, keep = _colour([[(SATURATION, 0.3)], [], [(CONTRAST, 1.3)], [(MATRIX, EYE), (BRIGHTNESS, 0.9)]])
    f = _fmt(E_F32)
    rs = Rs(32, 24, 0)
    with Handle(L, data) as H:
        idx = (C.c_int * m)(*index)
        geom, info, need = (Geom * m)(), (Info * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_col_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None,
                                            C.byref(col), geom, info, None, C.byref(need))
        assert rc == 0, ccmi.last_error()
        got = _plan(L, [data[i] for i in index], f, col, rects=rects, rs=rs)
        assert got[0] == 0, ccmi.last_error()
        for a, b in zip(geom, got[1]):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (32, 24)
        n0 = C.c_size_t(0)
        assert L.ccmi_latents_render_rs_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), geom, None,
                                             C.byref(n0)) == 0
        assert 256 < need.value - n0.value <= 256 * (-(-432 * m // 256) + 1)
        n1 = C.c_size_t(0)
        assert L.ccmi_latents_render_col_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              geom, None, None, C.byref(n1)) == 0
        assert n1.value == n0.value
