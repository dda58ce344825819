"""ccmi_decode_batch_dev_tone(_plan) / ccmi_latents_render_tone(_plan): the host side of the tone stage
(ccmi_tone, step 3x).  As tests/test_decode_filter_abi.py: no compute here, the plan calls are header-only,
the latent handles are plan-only, and the run entry point is only ever called with arguments the plan
rejects (made-up device pointers that nothing dereferences)."""
import ctypes as C

import pytest

from test_decode_colour_abi import BRIGHTNESS, CONTRAST, _colour
from test_decode_filter_abi import Filter, _filter, _ref, _same_plan
from test_decode_filter_abi import _plan as _plan_flt
from test_decode_resample_abi import (E_BF16, E_F32, ERR_ARG, FAKE, Geom, Handle, I, Info, P, Rect, Rs, Z, _args, _fields,
                                      _first, _fmt, _is_arg_error, _rects)
from test_decode_warp_abi import IDENT, _warp

T_BRIGHTNESS, T_SATURATION, T_CONTRAST, T_MATRIX, T_SOLARIZE, T_POSTERIZE, T_AUTOCONTRAST, T_EQUALIZE, T_SHARPNESS = range(9)
MAX_OPS = 8
NAMES = ("ccmi_decode_batch_dev_tone_plan", "ccmi_decode_batch_dev_tone", "ccmi_latents_render_tone_plan",
         "ccmi_latents_render_tone")


class ToneOp(C.Structure):
    _fields_ = [("op", C.c_int), ("v", C.c_float * 12)]


class Tone(C.Structure):
    _fields_ = [("count", C.c_void_p), ("ops", C.c_void_p)]


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.ccmi_decode_batch_dev_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_tone.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_render_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_tone.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_flt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_flt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for name in NAMES + ("ccmi_decode_batch_dev_flt_plan", "ccmi_latents_render_flt_plan", "ccmi_latents_decode",
                         "ccmi_decode_last_tail_groups"):
        getattr(lib, name).restype = C.c_int
    return lib


def _tone(frames):
    """frames: per frame a list of (op, value); value a number, 12 numbers, or None -> (ccmi_tone, keep)"""
    n = len(frames)
    count = (C.c_int * n)(*[len(f) for f in frames])
    flat = [o for f in frames for o in f]
    ops = (ToneOp * max(len(flat), 1))()
    for k, (op, value) in enumerate(flat):
        ops[k].op = op
        vals = [] if value is None else list(value) if hasattr(value, "__len__") else [value]
        for e, v in enumerate(vals):
            ops[k].v[e] = v
    return Tone(count=C.cast(count, C.c_void_p), ops=C.cast(ops, C.c_void_p)), (count, ops)


def _plan(lib, data, fmt, tone, flt=None, colour=None, rects=None, rs=None, warp=None, chroma=444, window=False):
    """(rc, geom, info, windows, workspace bytes) of ccmi_decode_batch_dev_tone_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_tone_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), _ref(warp),
                                             _ref(colour), _ref(tone), _ref(flt), geom, info, win if window else None,
                                             C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _run(lib, data, fmt, tone, flt=None, colour=None, rects=None, rs=None, warp=None, chroma=444):
    """ccmi_decode_batch_dev_tone with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*[FAKE + (i << 32) for i in range(n)])
    cp = (C.c_size_t * n)(*[1 << 30] * n)
    return lib.ccmi_decode_batch_dev_tone(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), _ref(rs), _ref(warp),
                                          _ref(colour), _ref(tone), _ref(flt), 0, chroma, None, 0, None)


def _rejected(lib, data, tone, frame, *words, **kw):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned or written"""
    rc, _, _, _, got = _plan(lib, data, _fmt(), tone, **kw)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    kw.pop("window", None)
    _is_arg_error(_run(lib, data, _fmt(), tone, **kw), frame, *words)


def _r256(v):
    return -(-v // 256) * 256


def _grow(staged_by_tone, staged, sharp, stats):
    """ccmi.h's formula over the _flt call of the same filter: the frames staged by their tone ops alone cost
    what a staged frame costs; then 512 per staged frame, a second frame per sharpness frame, 3328 per
    statistic op"""
    return (sum(_r256(12 * h * w) + 256 for h, w in staged_by_tone) + 512 * staged + sum(_r256(12 * h * w) for h, w in sharp)
            + 3328 * stats)


def test_symbols_and_struct_layout(L):
    import ccmi
    from ccmi import decode
    for name in NAMES:
        assert name in ccmi.EXPORTED and name in decode._PROTOS
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(ToneOp) == 52 and ToneOp.v.offset == 4
    assert C.sizeof(decode.ToneOp) == 52 and decode.ToneOp.v.offset == 4
    assert C.sizeof(Tone) == 2 * p and Tone.ops.offset == p
    assert C.sizeof(decode.Tone) == 2 * p and decode.Tone.ops.offset == p
    assert decode.TONE_MAX_OPS == MAX_OPS
    assert [decode.TONE_BRIGHTNESS, decode.TONE_SATURATION, decode.TONE_CONTRAST, decode.TONE_MATRIX, decode.TONE_SOLARIZE,
            decode.TONE_POSTERIZE, decode.TONE_AUTOCONTRAST, decode.TONE_EQUALIZE, decode.TONE_SHARPNESS] == list(range(9))


def test_count_or_ops_null_and_counts_outside_the_range(L, data):
    import ccmi
    t, keep = _tone([[(T_EQUALIZE, None)]] * 3)
    _rejected(L, data, Tone(count=None, ops=t.ops), 0, "counts")
    _rejected(L, data, Tone(count=t.count, ops=None), 0, "ops", "NULL")
    for bad in (-1, 9, 1 << 20):
        t, keep = _tone([[], [(T_EQUALIZE, None)], []])
        keep[0][2] = bad
        _rejected(L, data, t, 2, "tone ops", str(bad), "8")
    t, keep = _tone([[(T_AUTOCONTRAST, None)] * MAX_OPS] * 3)  # the longest list is fine
    rc, *_ = _plan(L, data, _fmt(), t)
    assert rc == 0, ccmi.last_error()


def test_unknown_op(L, data):
    for bad in (-1, 9, 1 << 20):
        t, keep = _tone([[(T_BRIGHTNESS, 1.0)], [(T_EQUALIZE, None), (bad, 1.0)], []])
        _rejected(L, data, t, 1, "tone op 1", "unknown op", str(bad))


@pytest.mark.parametrize("op", (T_BRIGHTNESS, T_SATURATION, T_CONTRAST, T_SHARPNESS))
@pytest.mark.parametrize("bad", (-0.5, float("nan"), float("inf"), -float("inf")))
def test_negative_or_non_finite_factor(L, data, op, bad):
    import ccmi
    t, keep = _tone([[], [], [(T_EQUALIZE, None), (op, bad)]])  # the flat array is walked by the frames' own counts
    _rejected(L, data, t, 2, "tone op 1", "factor")
    t, keep = _tone([[(op, 0.0)], [(op, -0.0)], [(op, 3e38)]])
    rc, *_ = _plan(L, data, _fmt(), t)
    assert rc == 0, ccmi.last_error()


def test_non_finite_matrix_entry_nan_threshold_and_posterize_bits(L, data):
    import ccmi
    for e in (0, 7, 11):
        m = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
        m[e] = float("inf") if e else float("nan")
        t, keep = _tone([[(T_MATRIX, m)], [], []])
        _rejected(L, data, t, 0, "matrix entry %d" % e, "finite")
    t, keep = _tone([[], [(T_SOLARIZE, float("nan"))], []])
    _rejected(L, data, t, 1, "threshold", "NaN")
    for bad in (0.0, 9.0, 2.5, -1.0, float("nan"), float("inf")):
        t, keep = _tone([[], [], [(T_POSTERIZE, bad)]])
        _rejected(L, data, t, 2, "posterize bits")
    t, keep = _tone([[(T_SOLARIZE, float("inf")), (T_SOLARIZE, -float("inf"))], [(T_POSTERIZE, 1.0)], [(T_POSTERIZE, 8.0)]])
    rc, *_ = _plan(L, data, _fmt(), t)
    assert rc == 0, ccmi.last_error()


def test_errors_on_every_geometry_with_colour_and_filter_and_from_a_handle(L, data):
    import ccmi
    bad, keep = _tone([[(T_EQUALIZE, None)], [(T_SHARPNESS, -1.0)]])
    good, keepg = _tone([[(T_EQUALIZE, None)], [(T_SHARPNESS, 1.0)]])
    w, keepw = _warp([IDENT] * 2, 8, 8)
    _rejected(L, data[:2], bad, 1, "factor", rects=[(0, 0, 16, 16)] * 2)
    _rejected(L, data[:2], bad, 1, "factor", rects=[(0, 0, 16, 16), (4, 4, 40, 20)], rs=Rs(out_w=8, out_h=8, filter=0))
    _rejected(L, data[:2], bad, 1, "factor", warp=w, window=True)
    # everything the _flt plan checks stays: a bad colour op, a bad filter, a bad geometry
    col, keepc = _colour([[(BRIGHTNESS, 1.0)], [(BRIGHTNESS, -2.0)]])
    _rejected(L, data[:2], good, 1, "colour op", "factor", colour=col)
    flt, keepf = _filter([[0.5, 0.25], [0.5, float("nan")]])
    _rejected(L, data[:2], good, 1, "tap 1", flt=flt)
    _rejected(L, data[:2], good, 0, "output size", rs=Rs(out_w=0, out_h=8, filter=0))
    _rejected(L, data[:2], good, 0, "resample", "warp", rs=Rs(8, 8, 0), warp=w)
    with Handle(L, data) as H:
        idx = (C.c_int * 2)(2, 0)
        geom, need = (Geom * 2)(), C.c_size_t(0)
        f = _fmt()
        rc = L.ccmi_latents_render_tone_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, None, C.byref(bad), None, geom,
                                             None, None, C.byref(need))
        _is_arg_error(rc, 1, "factor")
        assert need.value == 0
        op, cp = (C.c_void_p * 2)(FAKE, FAKE), (C.c_size_t * 2)(1 << 30, 1 << 30)
        rc = L.ccmi_latents_render_tone(H.h, idx, 2, None, op, cp, C.byref(f), None, None, None, C.byref(good), None, 0, 444,
                                        None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


def test_null_arguments(L, data):
    keep, sp, ln = _args(data)
    geom, need, win = (Geom * 3)(), C.c_size_t(0), (Rect * 3)()
    f = _fmt()
    t, keept = _tone([[(T_EQUALIZE, None)]] * 3)
    plan = L.ccmi_decode_batch_dev_tone_plan
    for args in ((sp, ln, 3, None, 0, 444, None, None, None, None, C.byref(t), None, geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(t), None, None, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(t), None, geom, None, win, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(t), None, geom, None, None, None)):
        _is_arg_error(plan(*args), 0, "null")
    a, b = C.c_int(7), C.c_int(7)  # a call that only plans reports no launches
    assert plan(sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, C.byref(t), None, geom, None, None, C.byref(need)) == 0
    assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def test_null_tone_and_all_counts_zero_plan_like_flt(L, data):
    """tone NULL and every count 0 (ops NULL allowed then): geometry, info, windows and workspace of the _flt
    plan, to the byte -- with and without colour ops and a filter, on every geometry."""
    import ccmi
    n = 3
    rects = [(16, 8, 64, 48), (100, 200, 300, 100), (0, 0, 32, 32)]
    none, keep0 = _tone([[], [], []])
    nullops = Tone(count=none.count, ops=None)
    col, keepc = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8)]])
    flt, keepf = _filter([[0.4, 0.2, 0.1], [], []], [2.0, 0.5, 2.0])
    f = _fmt(E_BF16)
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    cases = (dict(rects=None), dict(rects=[(16, 8, 64, 48)] * n), dict(rects=rects, rs=Rs(32, 24, 0)),
             dict(warp=w, window=True))
    for kw in cases:
        for c in (None, col):
            for fl in (None, flt):
                base = _plan_flt(L, data, f, fl, c, **kw)
                assert base[0] == 0, ccmi.last_error()
                for tone in (None, none, nullops):
                    got = _plan(L, data, f, tone, fl, c, **kw)
                    assert got[0] == 0, ccmi.last_error()
                    _same_plan(got, base, n)
                    assert got[3] == base[3] and got[4] == base[4]


def test_workspace_grows_by_the_documented_formula(L, data):
    """A mix of frames with no ops, pointwise ops only, statistics, sharpness, and filter only."""
    import ccmi
    n = 3
    f = _fmt(E_BF16)
    col, keepc = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8)]])
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    frame = [(240, 416), (720, 1280), (768, 512)]  # (h, w) of the three streams
    rects = [(16, 8, 65, 47), (100, 200, 301, 99), (0, 0, 33, 31)]
    region = [(r[3], r[2]) for r in rects]
    geoms = ((dict(rects=None), frame), (dict(rects=rects), region), (dict(rects=rects, rs=Rs(33, 21, 0)), [(21, 33)] * n),
             (dict(warp=w, window=True), [(16, 24)] * n))
    point = [(T_BRIGHTNESS, 1.1), (T_POSTERIZE, 4.0), (T_SOLARIZE, 0.5)]
    stats = [(T_EQUALIZE, None), (T_BRIGHTNESS, 0.9), (T_CONTRAST, 1.2), (T_AUTOCONTRAST, None), (T_EQUALIZE, None)]
    sharp = [(T_SHARPNESS, 1.5), (T_CONTRAST, 0.7), (T_SHARPNESS, 0.2)]
    t3 = [0.4, 0.2, 0.1]
    # (tone lists, filter taps, thresholds) -> frames staged by tone alone, staged frames, sharpness frames, statistic ops
    mixes = (([point, [], []], None, None, (0,), 1, (), 0),
             ([[], stats, sharp], None, None, (1, 2), 2, (2,), 5),
             ([point, [], stats], [[], t3, []], None, (0, 2), 3, (), 4),       # frame 1: filter only
             ([sharp, sharp, []], [t3, [], []], [2.0, 2.0, 0.5], (1,), 3, (0, 1), 2),
             ([[], [], [(T_SHARPNESS, 0.0)]], [[], [], []], [2.0, 2.0, 2.0], (2,), 1, (2,), 0))
    for kw, sizes in geoms:
        for c in (None, col):
            for tones, taps, th, by_tone, staged, sh, nstat in mixes:
                flt, keep = _filter(taps, th) if taps is not None else (None, None)
                base = _plan_flt(L, data, f, flt, c, **kw)
                assert base[0] == 0, ccmi.last_error()
                tone, keept = _tone(tones)
                got = _plan(L, data, f, tone, flt, c, **kw)
                assert got[0] == 0, ccmi.last_error()
                _same_plan(got, base, n)
                assert got[3] == base[3]
                want = _grow([sizes[j] for j in by_tone], staged, [sizes[j] for j in sh], nstat)
                assert got[4] - base[4] == want, (kw, tones, taps, th)


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    m = len(index)
    rects = [(0, 0, 64, 48), (640, 360, 200, 100), (16, 8, 100, 60), (3, 5, 40, 40)]
    tone, keep = _tone([[(T_EQUALIZE, None)], [], [(T_SHARPNESS, 2.0), (T_AUTOCONTRAST, None)], []])
    flt, keepf = _filter([[0.5, 0.25], [], [], [0.2] * 12], [2.0, 2.0, 0.5, 0.5])
    f = _fmt(E_F32)
    rs = Rs(32, 24, 0)
    with Handle(L, data) as H:
        idx = (C.c_int * m)(*index)
        geom, info, need = (Geom * m)(), (Info * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_tone_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                             C.byref(tone), C.byref(flt), geom, info, None, C.byref(need))
        assert rc == 0, ccmi.last_error()
        got = _plan(L, [data[i] for i in index], f, tone, flt, rects=rects, rs=rs)
        assert got[0] == 0, ccmi.last_error()
        for a, b in zip(geom, got[1]):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (32, 24)
        n0 = C.c_size_t(0)
        assert L.ccmi_latents_render_flt_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              C.byref(flt), geom, None, None, C.byref(n0)) == 0
        # the filter stages frames 0, 2 and 3; no frame is staged by its tone ops alone
        assert need.value - n0.value == _grow([], 3, [(24, 32)], 2)
        n1 = C.c_size_t(0)
        assert L.ccmi_latents_render_tone_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                               None, C.byref(flt), geom, None, None, C.byref(n1)) == 0
        assert n1.value == n0.value
