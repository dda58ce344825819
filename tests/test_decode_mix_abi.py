"""ccmi_decode_batch_dev_mix(_plan) / ccmi_latents_render_mix(_plan): the host side of the mix stage
(ccmi_mix, steps 4e and 4m).  As tests/test_decode_tone_abi.py: no compute here, the plan calls are
header-only, the latent handles are plan-only, and the run entry point is only ever called with arguments
the plan rejects (made-up device pointers that nothing dereferences)."""
import ctypes as C

import pytest

from test_decode_colour_abi import BRIGHTNESS, CONTRAST, _colour
from test_decode_filter_abi import _filter, _ref, _same_plan
from test_decode_resample_abi import (E_BF16, E_F32, ERR_ARG, FAKE, Geom, Handle, I, Info, P, Rect, Rs, Z, _args, _fields,
                                      _first, _fmt, _is_arg_error, _rects)
from test_decode_tone_abi import T_BRIGHTNESS, T_EQUALIZE, T_SHARPNESS, _tone
from test_decode_tone_abi import _plan as _plan_tone
from test_decode_warp_abi import IDENT, _warp

MAX_RECTS = 4
NAMES = ("ccmi_decode_batch_dev_mix_plan", "ccmi_decode_batch_dev_mix", "ccmi_latents_render_mix_plan",
         "ccmi_latents_render_mix")
NAN, INF = float("nan"), float("inf")


class EraseRect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int), ("v", C.c_float * 3), ("sigma", C.c_float)]


class Mix(C.Structure):
    _fields_ = [("count", C.c_void_p), ("rects", C.c_void_p), ("seed", C.c_void_p), ("partner", C.c_void_p),
                ("lam", C.c_void_p), ("box", C.c_void_p)]


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.ccmi_decode_batch_dev_mix_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_mix.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_render_mix_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_mix.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_tone_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for name in NAMES + ("ccmi_decode_batch_dev_tone_plan", "ccmi_latents_render_tone_plan", "ccmi_latents_decode",
                         "ccmi_decode_last_tail_groups"):
        getattr(lib, name).restype = C.c_int
    return lib


def _mix(n, erase=None, partner=None, lam=None, box=None, seed=None):
    """erase: per frame a list of (x, y, w, h, (v0, v1, v2), sigma); partner / lam / seed: per frame values;
    box: per frame (x, y, w, h); each None: the member is NULL -> (ccmi_mix, what it points to)"""
    keep = []

    def arr(ctype, vals):
        a = (ctype * max(len(vals), 1))(*vals)
        keep.append(a)
        return C.cast(a, C.c_void_p)
    m = Mix()
    if erase is not None:
        flat = [EraseRect(x, y, w, h, (C.c_float * 3)(*v), s) for f in erase for x, y, w, h, v, s in f]
        m.count = arr(C.c_int, [len(f) for f in erase])
        m.rects = arr(EraseRect, flat)
    if partner is not None:
        m.partner = arr(C.c_int, partner)
    if lam is not None:
        m.lam = arr(C.c_float, lam)
    if box is not None:
        m.box = arr(Rect, [Rect(*b) for b in box])
    if seed is not None:
        m.seed = arr(C.c_uint64, seed)
    return m, keep


def _plan(lib, data, fmt, mix, tone=None, flt=None, colour=None, rects=None, rs=None, warp=None, chroma=444, window=False):
    """(rc, geom, info, windows, workspace bytes) of ccmi_decode_batch_dev_mix_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_mix_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), _ref(warp),
                                            _ref(colour), _ref(tone), _ref(flt), _ref(mix), geom, info,
                                            win if window else None, C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _run(lib, data, fmt, mix, tone=None, flt=None, colour=None, rects=None, rs=None, warp=None, chroma=444):
    """ccmi_decode_batch_dev_mix with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*[FAKE + (i << 32) for i in range(n)])
    cp = (C.c_size_t * n)(*[1 << 30] * n)
    return lib.ccmi_decode_batch_dev_mix(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), _ref(rs), _ref(warp),
                                         _ref(colour), _ref(tone), _ref(flt), _ref(mix), 0, chroma, None, 0, None)


def _rejected(lib, data, mix, frame, *words, **kw):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned or written"""
    rc, _, _, _, got = _plan(lib, data, _fmt(), mix, **kw)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    kw.pop("window", None)
    _is_arg_error(_run(lib, data, _fmt(), mix, **kw), frame, *words)


def _accepted(lib, data, mix, **kw):
    import ccmi
    got = _plan(lib, data, _fmt(), mix, **kw)
    assert got[0] == 0, ccmi.last_error()
    return got


def _r256(v):
    return -(-v // 256) * 256


def _grow(staged, filtered):
    """ccmi.h's formula over the _tone call in which the M frames take the filter stage: 256 per mix-staged
    frame, and a second float32 frame per mix-staged frame with a radius or a solarize"""
    return 256 * staged + sum(_r256(12 * h * w) for h, w in filtered)


R0 = (2, 3, 5, 4, (0.5, -1.0, 2.0), 0.0)


def test_symbols_and_struct_layout(L):
    import ccmi
    from ccmi import decode
    for name in NAMES:
        assert name in ccmi.EXPORTED and name in decode._PROTOS
    p = C.sizeof(C.c_void_p)
    for rect in (EraseRect, decode.EraseRect):
        assert C.sizeof(rect) == 32 and rect.v.offset == 16 and rect.sigma.offset == 28
    for mix in (Mix, decode.Mix):
        assert C.sizeof(mix) == 6 * p
        assert [getattr(mix, k).offset for k in ("count", "rects", "seed", "partner", "lam", "box")] == [i * p for i in range(6)]
    assert decode.MIX_MAX_RECTS == MAX_RECTS


def test_null_mix_and_idle_mix_plan_like_tone(L, data):
    """mix NULL, every member NULL, and members that make no frame take the stage (counts 0, partners -1, with
    lam, boxes and seeds given or not): geometry, info, windows and workspace of the _tone plan, to the byte --
    with and without colour ops, tone ops and a filter, on every geometry."""
    import ccmi
    n = 3
    rects = [(16, 8, 64, 48), (100, 200, 300, 100), (0, 0, 32, 32)]
    idle = [_mix(n)[0], _mix(n, erase=[[], [], []])[0], _mix(n, partner=[-1] * n)[0]]
    full, keep = _mix(n, erase=[[], [], []], partner=[-1] * n, lam=[0.5] * n, box=[(1, 1, 4, 4)] * n, seed=[7] * n)
    col, keepc = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8)]])
    flt, keepf = _filter([[0.4, 0.2, 0.1], [], []], [2.0, 0.5, 2.0])
    tone, keept = _tone([[(T_EQUALIZE, None)], [], [(T_SHARPNESS, 1.5)]])
    f = _fmt(E_BF16)
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    cases = (dict(rects=None), dict(rects=[(16, 8, 64, 48)] * n), dict(rects=rects, rs=Rs(32, 24, 0)),
             dict(warp=w, window=True))
    for kw in cases:
        for c, t, fl in ((None, None, None), (col, None, flt), (None, tone, None), (col, tone, flt)):
            base = _plan_tone(L, data, f, t, fl, c, **kw)
            assert base[0] == 0, ccmi.last_error()
            for mix in [None, full] + idle:
                got = _plan(L, data, f, mix, t, fl, c, **kw)
                assert got[0] == 0, ccmi.last_error()
                _same_plan(got, base, n)
                assert got[3] == base[3] and got[4] == base[4]


def test_workspace_grows_by_the_documented_formula(L, data):
    """Takers, partner-only frames and untouched frames, with and without blur, solarize and tone ops, on
    region, size= and affine= geometries.  The base is the _tone call in which the mix-staged frames take the
    filter stage as well: those that do not already are given a solarize threshold of 1.0 there."""
    import ccmi
    n = 3
    f = _fmt(E_BF16)
    col, keepc = _colour([[(BRIGHTNESS, 1.2)], [], [(CONTRAST, 0.8)]])
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    geoms = ((dict(rects=[(16, 8, 65, 47)] * n), [(47, 65)] * n),
             (dict(rects=[(16, 8, 65, 47), (100, 200, 301, 99), (0, 0, 33, 31)], rs=Rs(33, 21, 0)), [(21, 33)] * n),
             (dict(warp=w, window=True), [(16, 24)] * n))
    t3 = [0.4, 0.2, 0.1]
    point = [(T_BRIGHTNESS, 1.1)]
    sharp = [(T_SHARPNESS, 1.5), (T_EQUALIZE, None)]
    # (erase, partner, tone lists, taps, thresholds) -> the mix-staged frames, those of them with a radius or a solarize
    cases = (([[R0], [], []], None, None, None, None, (0,), ()),                              # one taker, two untouched
             (None, [-1, 0, -1], None, None, None, (0, 1), ()),                               # frame 0 is a partner only
             ([[], [R0] * 4, []], [2, -1, 2], None, [t3, [], []], [2.0, 2.0, 0.5], (0, 1, 2), (0, 2)),
             ([[R0], [], []], [-1, -1, 1], [point, sharp, []], None, None, (0, 1, 2), ()),
             ([[], [], [R0]], [1, -1, -1], [sharp, [], point], [[], t3, []], [0.5, 2.0, 2.0], (0, 1, 2), (0, 1)),
             (None, [0, -1, -1], [[], sharp, []], [[], t3, t3], None, (0,), ()))                # frame 0 mixes with itself
    for kw, sizes in geoms:
        for c in (None, col):
            for erase, partner, tones, taps, th, staged, filtered in cases:
                mix, keepm = _mix(n, erase=erase, partner=partner, lam=[0.3] * n)
                tone, keept = _tone(tones) if tones is not None else (None, None)
                flt, keepf = _filter(taps, th) if taps is not None else (None, None)
                # the base: the same call without mix, the staged frames taking the filter stage
                bth = list(th) if th is not None else [2.0] * n
                takes = [taps is not None and len(taps[j]) > 1 or bth[j] <= 1.0 for j in range(n)]
                for j in staged:
                    if not takes[j]:
                        bth[j] = 1.0
                bflt, keepb = _filter(taps if taps is not None else [[]] * n, bth)
                base = _plan_tone(L, data, f, tone, bflt, c, **kw)
                assert base[0] == 0, ccmi.last_error()
                got = _plan(L, data, f, mix, tone, flt, c, **kw)
                assert got[0] == 0, ccmi.last_error()
                _same_plan(got, base, n)
                assert got[3] == base[3]
                assert [j for j in staged if takes[j]] == list(filtered)
                assert got[4] - base[4] == _grow(len(staged), [sizes[j] for j in filtered]), (kw, erase, partner, tones, taps, th)


def test_counts_and_rects(L, data):
    for bad in (-1, 5, 1 << 20):
        m, keep = _mix(3, erase=[[], [R0], []])
        keep[0][2] = bad
        _rejected(L, data, m, 2, "erase rectangles", str(bad), "4")
    m, keep = _mix(3, erase=[[], [R0], []])
    m.rects = None
    _rejected(L, data, m, 1, "rectangles", "NULL")
    _accepted(L, data, _mix(3, erase=[[R0] * MAX_RECTS] * 3)[0], rects=[(0, 0, 16, 16)] * 3)  # the longest list is fine


@pytest.mark.parametrize("bad", (NAN, INF, -INF))
def test_non_finite_value_or_sigma_and_negative_sigma(L, data, bad):
    for c in range(3):
        v = [0.0, 0.0, 0.0]
        v[c] = bad
        m, keep = _mix(3, erase=[[], [R0, (0, 0, 1, 1, tuple(v), 0.0)], []])  # the flat array is walked by the frames' own counts
        _rejected(L, data, m, 1, "rectangle 1", "value %d" % c, "finite")
    m, keep = _mix(3, erase=[[], [], [(0, 0, 1, 1, (0, 0, 0), bad)]])
    _rejected(L, data, m, 2, "rectangle 0", "sigma")
    m, keep = _mix(3, erase=[[(0, 0, 1, 1, (0, 0, 0), -0.5)], [], []])
    _rejected(L, data, m, 0, "rectangle 0", "sigma")
    _accepted(L, data, _mix(3, erase=[[(0, 0, 1, 1, (3e38, -3e38, -0.0), 3e38)], [], []])[0])


def test_rectangles_and_boxes_negative_or_outside_the_frame(L, data):
    kw = dict(rects=[(16, 8, 21, 37)] * 3)  # every frame is stored at 37 rows x 21 columns
    for x, y, w, h, word in ((0, 0, -1, 4, "negative"), (0, 0, 4, -1, "negative"), (-1, 0, 4, 4, "outside"), (0, -1, 4, 4, "outside"),
                             (18, 0, 4, 4, "outside"), (0, 34, 4, 4, "outside"), (0, 0, 22, 1, "outside"), (0, 0, 1, 38, "outside"),
                             (21, 0, 1, 1, "outside"), (2 ** 31 - 1, 0, 2, 1, "outside")):
        m, keep = _mix(3, erase=[[], [R0, (x, y, w, h, (0, 0, 0), 0.0)], []])
        _rejected(L, data, m, 1, "rectangle 1", word, **kw)
        m, keep = _mix(3, partner=[-1, -1, 0], lam=[0.5] * 3, box=[(0, 0, 0, 0), (0, 0, 0, 0), (x, y, w, h)])
        _rejected(L, data, m, 2, "box", word, **kw)
    # empty ones are legal wherever they lie; the whole frame, a corner pixel and the last row are inside
    ok = [(50, 50, 0, 4, (0, 0, 0), 0.0), (-5, -5, 3, 0, (0, 0, 0), 1.0), (0, 0, 21, 37, (0, 0, 0), 0.0), (20, 36, 1, 1, (0, 0, 0), 0.0)]
    _accepted(L, data, _mix(3, erase=[ok, [], []], partner=[1, 2, 0], lam=[0.5] * 3,
                            box=[(0, 0, 21, 37), (99, 99, 0, 0), (20, 36, 1, 1)])[0], **kw)
    # the stored size is the output size with a resample or a warp
    m, keep = _mix(3, erase=[[], [], [(0, 0, 9, 8, (0, 0, 0), 0.0)]])
    _rejected(L, data, m, 2, "rectangle 0", "outside", rs=Rs(8, 8, 0), **kw)
    w, keepw = _warp([IDENT] * 3, 8, 8)
    _rejected(L, data, m, 2, "rectangle 0", "outside", warp=w, window=True)
    _accepted(L, data, _mix(3, erase=[[], [], [(0, 0, 8, 8, (0, 0, 0), 0.0)]])[0], rs=Rs(8, 8, 0), **kw)


def test_partner_outside_the_call_or_of_another_size(L, data):
    for bad in (-2, 3, 1 << 20):
        m, keep = _mix(3, partner=[-1, bad, -1], lam=[0.5] * 3)
        _rejected(L, data, m, 1, "partner", str(bad))
    m, keep = _mix(3, partner=[-1, -1, 0], lam=[0.5] * 3)
    _rejected(L, data, m, 2, "partner 0", "416 x 240", "512 x 768")  # whole frames of three sizes
    _rejected(L, data, m, 2, "partner 0", rects=[(0, 0, 16, 16), (0, 0, 16, 16), (0, 0, 16, 18)])
    _accepted(L, data, m, rects=[(0, 0, 16, 18), (0, 0, 20, 20), (4, 4, 16, 18)])
    _accepted(L, data, m, rects=[(0, 0, 16, 16), (0, 0, 20, 20), (4, 4, 16, 18)], rs=Rs(8, 8, 0))


def test_lam_null_nan_or_outside_the_unit_interval(L, data):
    kw = dict(rects=[(0, 0, 16, 16)] * 3)
    m, keep = _mix(3, partner=[-1, 0, -1])
    _rejected(L, data, m, 1, "lam", "NULL", **kw)
    for bad in (NAN, -0.25, 1.5, INF, -INF):
        m, keep = _mix(3, partner=[-1, -1, 1], lam=[bad, bad, bad])
        _rejected(L, data, m, 2, "lam", **kw)
        # lam is read only where a frame blends: not without a partner, not with a box
        _accepted(L, data, _mix(3, partner=[-1, -1, 1], lam=[bad, bad, 0.5])[0], **kw)
        _accepted(L, data, _mix(3, partner=[-1, -1, 1], lam=[bad] * 3, box=[(0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 2, 2)])[0], **kw)
    _accepted(L, data, _mix(3, partner=[-1, -1, 1], box=[(0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 2, 2)])[0], **kw)  # lam NULL, a box
    for ok in (0.0, -0.0, 1.0):
        _accepted(L, data, _mix(3, partner=[2, 2, 2], lam=[ok] * 3)[0], **kw)


def test_errors_with_colour_tone_and_filter_and_from_a_handle(L, data):
    import ccmi
    bad, keep = _mix(2, erase=[[R0], [(0, 0, 1, 1, (NAN, 0, 0), 0.0)]])
    good, keepg = _mix(2, erase=[[R0], []], partner=[1, -1], lam=[0.5, 0.5])
    w, keepw = _warp([IDENT] * 2, 8, 8)
    _rejected(L, data[:2], bad, 1, "value 0", rects=[(0, 0, 16, 16)] * 2)
    _rejected(L, data[:2], bad, 1, "value 0", rects=[(0, 0, 16, 16), (4, 4, 40, 20)], rs=Rs(out_w=8, out_h=8, filter=0))
    _rejected(L, data[:2], bad, 1, "value 0", warp=w, window=True)
    # everything the _tone plan checks stays: a bad colour op, tone op, filter or geometry
    kw = dict(rects=[(0, 0, 16, 16)] * 2)
    col, keepc = _colour([[(BRIGHTNESS, 1.0)], [(BRIGHTNESS, -2.0)]])
    _rejected(L, data[:2], good, 1, "colour op", "factor", colour=col, **kw)
    tone, keept = _tone([[(T_EQUALIZE, None)], [(T_SHARPNESS, -1.0)]])
    _rejected(L, data[:2], good, 1, "tone op", "factor", tone=tone, **kw)
    flt, keepf = _filter([[0.5, 0.25], [0.5, NAN]])
    _rejected(L, data[:2], good, 1, "tap 1", flt=flt, **kw)
    _rejected(L, data[:2], good, 0, "output size", rs=Rs(out_w=0, out_h=8, filter=0), **kw)
    _rejected(L, data[:2], good, 0, "resample", "warp", rs=Rs(8, 8, 0), warp=w)
    with Handle(L, data) as H:
        idx = (C.c_int * 2)(2, 0)
        geom, need = (Geom * 2)(), C.c_size_t(0)
        f = _fmt()
        rc = L.ccmi_latents_render_mix_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(bad),
                                            geom, None, None, C.byref(need))
        _is_arg_error(rc, 1, "value 0")
        assert need.value == 0
        rc = L.ccmi_latents_render_mix_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(good),
                                            geom, None, None, C.byref(need))
        _is_arg_error(rc, 0, "partner 1")  # frames 2 and 0 of the handle: a Kodak frame and a class D one
        op, cp = (C.c_void_p * 2)(FAKE, FAKE), (C.c_size_t * 2)(1 << 30, 1 << 30)
        rc = L.ccmi_latents_render_mix(H.h, idx, 2, None, op, cp, C.byref(f), None, None, None, None, None, C.byref(good), 0,
                                       444, None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


def test_null_arguments_and_mix_without_a_format(L, data):
    keep, sp, ln = _args(data)
    geom, need, win = (Geom * 3)(), C.c_size_t(0), (Rect * 3)()
    f = _fmt()
    m, keepm = _mix(3, erase=[[R0], [], []])
    plan = L.ccmi_decode_batch_dev_mix_plan
    for args in ((sp, ln, 3, None, 0, 444, None, None, None, None, None, None, C.byref(m), geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(m), None, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(m), geom, None, win, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(m), geom, None, None, None)):
        _is_arg_error(plan(*args), 0, "null")
    op, cp = (C.c_void_p * 3)(FAKE, FAKE, FAKE), (C.c_size_t * 3)(1 << 30, 1 << 30, 1 << 30)
    rc = L.ccmi_decode_batch_dev_mix(sp, ln, 3, None, op, cp, None, None, None, None, None, None, C.byref(m), 0, 444, None, 0, None)
    _is_arg_error(rc, 0, "null")  # mix without a format
    a, b = C.c_int(7), C.c_int(7)  # a call that only plans reports no launches
    assert plan(sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(m), geom, None, None, C.byref(need)) == 0
    assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    m = len(index)
    rects = [(0, 0, 64, 48), (640, 360, 200, 100), (16, 8, 100, 60), (3, 5, 40, 40)]
    mix, keep = _mix(m, erase=[[R0], [], [], []], partner=[-1, -1, 3, -1], lam=[0.5] * m, seed=[1, 2, 3, 4])
    tone, keept = _tone([[(T_EQUALIZE, None)], [], [(T_SHARPNESS, 2.0)], []])
    flt, keepf = _filter([[0.5, 0.25], [], [], []], [2.0, 2.0, 2.0, 2.0])
    f = _fmt(E_F32)
    rs = Rs(32, 24, 0)
    with Handle(L, data) as H:
        idx = (C.c_int * m)(*index)
        geom, info, need = (Geom * m)(), (Info * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_mix_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                            C.byref(tone), C.byref(flt), C.byref(mix), geom, info, None, C.byref(need))
        assert rc == 0, ccmi.last_error()
        got = _plan(L, [data[i] for i in index], f, mix, tone, flt, rects=rects, rs=rs)
        assert got[0] == 0, ccmi.last_error()
        for a, b in zip(geom, got[1]):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (32, 24)
        # the base: frames 0, 2 and 3 are mix-staged; 0 and 2 take the stage already, 3 is given a solarize of 1.0
        bflt, keepb = _filter([[0.5, 0.25], [], [], []], [2.0, 2.0, 2.0, 1.0])
        n0 = C.c_size_t(0)
        assert L.ccmi_latents_render_tone_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                               C.byref(tone), C.byref(bflt), geom, None, None, C.byref(n0)) == 0
        assert need.value - n0.value == _grow(3, [(24, 32)])
        n1 = C.c_size_t(0)
        assert L.ccmi_latents_render_mix_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              C.byref(tone), C.byref(bflt), None, geom, None, None, C.byref(n1)) == 0
        assert n1.value == n0.value
