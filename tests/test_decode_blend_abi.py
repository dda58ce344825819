"""ccmi_decode_batch_dev_blend(_plan) / ccmi_latents_render_blend(_plan): the host side of the blend stage
(ccmi_blend, step 3b).  As tests/test_decode_mix_abi.py: no compute here, the plan calls are header-only, the
latent handles are plan-only, and the run entry point is only ever called with arguments the plan rejects
(made-up device pointers that nothing dereferences)."""
import ctypes as C

import pytest

from test_decode_filter_abi import _filter, _ref, _same_plan
from test_decode_mix_abi import R0, _grow, _mix
from test_decode_mix_abi import _plan as _plan_mix
from test_decode_resample_abi import (E_BF16, E_F32, ERR_ARG, FAKE, Geom, Handle, I, Info, P, Rect, Rs, Z, _args, _fields,
                                      _first, _fmt, _is_arg_error, _rects)
from test_decode_tone_abi import T_EQUALIZE, T_SHARPNESS, _tone
from test_decode_warp_abi import IDENT, _warp

MAX_TERMS = 8
NAMES = ("ccmi_decode_batch_dev_blend_plan", "ccmi_decode_batch_dev_blend", "ccmi_latents_render_blend_plan",
         "ccmi_latents_render_blend")
NAN, INF = float("nan"), float("inf")


class Blend(C.Structure):
    _fields_ = [("count", C.c_void_p), ("source", C.c_void_p), ("weight", C.c_void_p), ("silent", C.c_void_p)]


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.ccmi_decode_batch_dev_blend_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_blend.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_render_blend_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_blend.argtypes = [P, P, I, P, P, P, P, P, P, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_mix_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_render_mix_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    for name in NAMES + ("ccmi_decode_batch_dev_mix_plan", "ccmi_latents_render_mix_plan", "ccmi_latents_decode"):
        getattr(lib, name).restype = C.c_int
    return lib


def _blend(n, terms=None, silent=None):
    """terms: per frame a list of (source, weight); silent: per frame flags; each None: the members are NULL
    -> (ccmi_blend, what it points to)"""
    keep = []

    def arr(ctype, vals):
        a = (ctype * max(len(vals), 1))(*vals)
        keep.append(a)
        return C.cast(a, C.c_void_p)
    b = Blend()
    if terms is not None:
        b.count = arr(C.c_int, [len(f) for f in terms])
        b.source = arr(C.c_int, [s for f in terms for s, _ in f])
        b.weight = arr(C.c_float, [w for f in terms for _, w in f])
    if silent is not None:
        b.silent = arr(C.c_int, [int(v) for v in silent])
    return b, keep


def _plan(lib, data, fmt, blend, mix=None, tone=None, flt=None, rects=None, rs=None, warp=None, chroma=444, window=False):
    """(rc, geom, info, windows, workspace bytes) of ccmi_decode_batch_dev_blend_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, win, need = (Geom * n)(), (Info * n)(), (Rect * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_blend_plan(sp, ln, n, _rects(rects, n), 0, chroma, C.byref(fmt), _ref(rs), _ref(warp),
                                              None, _ref(tone), _ref(flt), _ref(blend), _ref(mix), geom, info,
                                              win if window else None, C.byref(need))
    return rc, geom, info, [(r.x, r.y, r.w, r.h) for r in win], need.value


def _run(lib, data, fmt, blend, mix=None, tone=None, flt=None, rects=None, rs=None, warp=None, chroma=444, outs=None):
    """ccmi_decode_batch_dev_blend with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*(outs if outs is not None else [FAKE + (i << 32) for i in range(n)]))
    cp = (C.c_size_t * n)(*[1 << 30] * n)
    return lib.ccmi_decode_batch_dev_blend(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), _ref(rs), _ref(warp), None,
                                           _ref(tone), _ref(flt), _ref(blend), _ref(mix), 0, chroma, None, 0, None)


def _rejected(lib, data, blend, frame, *words, **kw):
    """the plan and the run entry point both refuse, naming the frame; nothing is planned or written"""
    rc, _, _, _, got = _plan(lib, data, _fmt(), blend, **kw)
    _is_arg_error(rc, frame, *words)
    assert got == 0
    kw.pop("window", None)
    _is_arg_error(_run(lib, data, _fmt(), blend, **kw), frame, *words)


def _accepted(lib, data, blend, **kw):
    import ccmi
    got = _plan(lib, data, _fmt(), blend, **kw)
    assert got[0] == 0, ccmi.last_error()
    return got


SAME = dict(rects=[(16, 8, 21, 37)] * 3)  # every frame is stored at 37 rows x 21 columns


def test_symbols_and_struct_layout(L):
    import ccmi
    from ccmi import decode
    for name in NAMES:
        assert name in ccmi.EXPORTED and name in decode._PROTOS
    p = C.sizeof(C.c_void_p)
    for blend in (Blend, decode.Blend):
        assert C.sizeof(blend) == 4 * p
        assert [getattr(blend, k).offset for k in ("count", "source", "weight", "silent")] == [i * p for i in range(4)]
    assert decode.BLEND_MAX_TERMS == MAX_TERMS


def test_null_blend_and_idle_blend_plan_like_mix(L, data):
    """blend NULL, every member NULL, and members that give no frame terms and make none silent (counts 0,
    flags 0, with sources and weights given or not): geometry, info, windows and workspace of the _mix plan, to
    the byte -- with and without a mix, tone ops and a filter, on every geometry."""
    import ccmi
    n = 3
    idle = [None, _blend(n)[0], _blend(n, terms=[[], [], []])[0], _blend(n, silent=[0] * n)[0],
            _blend(n, terms=[[], [], []], silent=[0] * n)[0]]
    full, keep = _blend(n, terms=[[], [], []], silent=[0] * n)
    spare = (C.c_int * 4)(0, 1, 2, 0), (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)  # given, and read by no frame
    full.source, full.weight = C.cast(spare[0], C.c_void_p), C.cast(spare[1], C.c_void_p)
    mix, keepm = _mix(n, erase=[[R0], [], []], partner=[-1, 0, -1], lam=[0.3] * n)
    flt, keepf = _filter([[0.4, 0.2, 0.1], [], []], [2.0, 0.5, 2.0])
    tone, keept = _tone([[(T_EQUALIZE, None)], [], [(T_SHARPNESS, 1.5)]])
    f = _fmt(E_BF16)
    w, keepw = _warp([IDENT, (0.5, 0.1, 600, -0.1, 0.5, 300), (0, -1, 300, 1, 0, 20)], 24, 16)
    cases = (dict(rects=[(16, 8, 64, 48)] * n), dict(rects=[(16, 8, 64, 48), (100, 200, 300, 100), (0, 0, 32, 32)], rs=Rs(32, 24, 0)),
             dict(warp=w, window=True))
    for kw in cases:
        for m, t, fl in ((None, None, None), (mix, None, flt), (None, tone, None), (mix, tone, flt)):
            base = _plan_mix(L, data, f, m, t, fl, None, **kw)
            assert base[0] == 0, ccmi.last_error()
            for blend in idle + [full]:
                got = _plan(L, data, f, blend, m, t, fl, **kw)
                assert got[0] == 0, ccmi.last_error()
                _same_plan(got, base, n)
                assert got[3] == base[3] and got[4] == base[4]


def test_workspace_grows_by_the_documented_formula(L, data):
    """ccmi.h: the _mix call in which the blend-staged frames are mix-staged, plus 256 ceil(|M| / 4) bytes.  The
    base is the _mix call that mix-stages the same frames M by other means: a frame of M that `mix` does not
    stage is made its own MixUp partner with lam 1 there (mix-staged, and nothing else).  Without a mix and a
    filter the growth over the plain call is also spelled out: staging, mix table, blend table."""
    import ccmi
    f = _fmt(E_BF16)
    t3 = [0.4, 0.2, 0.1]
    for n, sizes, kw in ((3, [(37, 21)] * 3, SAME), (6, [(24, 32)] * 6, dict(rects=[(0, 0, 40 + j, 30 + j) for j in range(6)], rs=Rs(32, 24, 0)))):
        d = [data[j % 3] for j in range(n)]
        # (terms, silent, the mix's partners or None, taps, thresholds) -> M
        cases = [([[(1, 0.5), (2, 0.5)]] + [[]] * (n - 1), [0, 1, 1] + [0] * (n - 3), None, None, None, (0, 1, 2)),
                 ([[]] * (n - 1) + [[(n - 1, 1.0)]], None, None, None, None, (n - 1,)),
                 (None, [0, 1] + [0] * (n - 2), None, None, None, (1,)),                    # a silent frame nobody reads
                 ([[(0, 1.0)] * 8] + [[]] * (n - 1), None, [-1, -1, 1] + [-1] * (n - 3), [t3] + [[]] * (n - 1), [2.0, 0.5] + [2.0] * (n - 2), (0, 1, 2)),
                 ([[(j, 0.25)] for j in range(n)], None, None, None, None, tuple(range(n)))]
        for terms, silent, partner, taps, th, staged in cases:
            blend, keepb = _blend(n, terms=terms, silent=silent)
            mix, keepm = _mix(n, partner=partner, lam=[0.3] * n) if partner is not None else (None, None)
            flt, keepf = _filter(taps, th) if taps is not None else (None, None)
            bp = list(partner) if partner is not None else [-1] * n
            lam = [0.3] * n
            for j in staged:
                if bp[j] < 0 and j not in bp:
                    bp[j], lam[j] = j, 1.0
            bmix, keepx = _mix(n, partner=bp, lam=lam)
            base = _plan_mix(L, d, f, bmix, None, flt, None, **kw)
            assert base[0] == 0, ccmi.last_error()
            got = _plan(L, d, f, blend, mix, None, flt, **kw)
            assert got[0] == 0, ccmi.last_error()
            _same_plan(got, base, n)
            assert got[4] - base[4] == 256 * -(-len(staged) // 4), (n, terms, silent, partner)
            # and against the _mix call without the stage: the mix stage's own formula over M
            if partner is None and taps is None:
                plain = _plan_mix(L, d, f, None, None, None, None, **kw)
                staging = sum(-(-12 * sizes[j][0] * sizes[j][1] // 256) * 256 + 256 for j in staged)
                assert got[4] - plain[4] == staging + _grow(len(staged), []) + 256 * -(-len(staged) // 4)


def test_counts_sources_and_weights(L, data):
    for bad in (-1, 9, 1 << 20):
        b, keep = _blend(3, terms=[[], [(0, 1.0)], []])
        keep[0][1] = bad
        _rejected(L, data, b, 1, "blend terms", str(bad), "8", **SAME)
    for member in ("source", "weight"):
        b, keep = _blend(3, terms=[[], [], [(0, 1.0)]])
        setattr(b, member, None)
        _rejected(L, data, b, 2, "blend", "NULL", **SAME)
    for bad in (-1, 3, 1 << 20):
        b, keep = _blend(3, terms=[[(0, 1.0)], [(1, 0.5), (bad, 0.5)], []])  # the flat arrays are walked by the frames' own counts
        _rejected(L, data, b, 1, "term 1", "source", str(bad), **SAME)
    for bad in (NAN, INF, -INF):
        b, keep = _blend(3, terms=[[], [(1, 0.5)], [(0, 1.0), (1, 0.0), (2, bad)]])
        _rejected(L, data, b, 2, "term 2", "weight", "finite", **SAME)
    # the longest list, a frame as its own source, one source eight times, weights 0, negative, huge, not summing to 1
    _accepted(L, data, _blend(3, terms=[[(0, 1.0)] * MAX_TERMS, [(1, -2.5), (1, 0.0), (0, 3e38)], [(2, -0.0)]])[0], **SAME)


def test_source_of_another_stored_size(L, data):
    b, keep = _blend(3, terms=[[], [], [(2, 0.5), (0, 0.5)]])
    _rejected(L, data, b, 2, "term 1", "source 0", "416 x 240", "512 x 768")  # whole frames of three sizes
    _rejected(L, data, b, 2, "term 1", "source 0", rects=[(0, 0, 16, 16), (0, 0, 16, 16), (0, 0, 16, 18)])
    _accepted(L, data, b, rects=[(0, 0, 16, 18), (0, 0, 20, 20), (4, 4, 16, 18)])
    _accepted(L, data, b, rects=[(0, 0, 16, 16), (0, 0, 20, 20), (4, 4, 16, 18)], rs=Rs(8, 8, 0))
    w, keepw = _warp([IDENT] * 3, 8, 8)
    _accepted(L, data, b, warp=w, window=True)


def test_silent_frames(L, data):
    b, keep = _blend(3, terms=[[(1, 1.0)], [(0, 1.0)], []], silent=[0, 1, 0])
    _rejected(L, data, b, 1, "silent", "terms", **SAME)
    b, keep = _blend(3, terms=[[(1, 1.0)], [], []], silent=[0, 1, 0])
    m, keepm = _mix(3, erase=[[], [R0], []])
    _rejected(L, data, b, 1, "silent", "rectangles", mix=m, **SAME)
    m, keepm = _mix(3, partner=[-1, 2, -1], lam=[0.5] * 3)
    _rejected(L, data, b, 1, "silent", "partner", mix=m, **SAME)
    # a silent frame may be a partner and a source, and its geometry is reported like any other's
    m, keepm = _mix(3, partner=[1, -1, 1], lam=[0.5] * 3)
    got = _accepted(L, data, b, mix=m, **SAME)
    assert [(g.width, g.height, g.elems) for g in got[1]] == [(21, 37, 3 * 21 * 37)] * 3
    # run calls: a silent frame's output may be NULL, another frame's may not
    import ccmi
    rc = _run(L, data, _fmt(), b, outs=[0, 0, FAKE], **SAME)
    _is_arg_error(rc, 0, "NULL")
    rc = _run(L, data, _fmt(), b, outs=[FAKE, 0, 0], **SAME)
    _is_arg_error(rc, 2, "NULL")


def test_blend_without_a_format_and_null_arguments(L, data):
    keep, sp, ln = _args(data)
    geom, need, win = (Geom * 3)(), C.c_size_t(0), (Rect * 3)()
    f = _fmt()
    b, keepb = _blend(3, terms=[[(0, 1.0)], [], []])
    plan = L.ccmi_decode_batch_dev_blend_plan
    for args in ((sp, ln, 3, None, 0, 444, None, None, None, None, None, None, C.byref(b), None, geom, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(b), None, None, None, None, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(b), None, geom, None, win, C.byref(need)),
                 (sp, ln, 3, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(b), None, geom, None, None, None)):
        _is_arg_error(plan(*args), 0, "null")
    op, cp = (C.c_void_p * 3)(FAKE, FAKE, FAKE), (C.c_size_t * 3)(1 << 30, 1 << 30, 1 << 30)
    rc = L.ccmi_decode_batch_dev_blend(sp, ln, 3, None, op, cp, None, None, None, None, None, None, C.byref(b), None, 0, 444,
                                       None, 0, None)
    _is_arg_error(rc, 0, "null")  # blend without a format


def test_errors_with_mix_tone_and_filter_and_from_a_handle(L, data):
    import ccmi
    kw = dict(rects=[(0, 0, 16, 16)] * 2)
    bad, keep = _blend(2, terms=[[(0, 0.5)], [(0, 0.5), (1, NAN)]])
    good, keepg = _blend(2, terms=[[(0, 0.5), (1, 0.5)], []], silent=[0, 1])
    _rejected(L, data[:2], bad, 1, "term 1", "weight", **kw)
    _rejected(L, data[:2], bad, 1, "term 1", "weight", rects=[(0, 0, 16, 16), (4, 4, 40, 20)], rs=Rs(out_w=8, out_h=8, filter=0))
    # everything the _mix plan checks stays: a bad mix, tone op, filter or geometry
    m, keepm = _mix(2, partner=[5, -1], lam=[0.5] * 2)
    _rejected(L, data[:2], good, 0, "partner", "5", mix=m, **kw)
    tone, keept = _tone([[(T_EQUALIZE, None)], [(T_SHARPNESS, -1.0)]])
    _rejected(L, data[:2], good, 1, "tone op", "factor", tone=tone, **kw)
    flt, keepf = _filter([[0.5, 0.25], [0.5, NAN]])
    _rejected(L, data[:2], good, 1, "tap 1", flt=flt, **kw)
    _rejected(L, data[:2], good, 0, "output size", rs=Rs(out_w=0, out_h=8, filter=0), **kw)
    with Handle(L, data) as H:
        idx = (C.c_int * 2)(2, 0)
        geom, need = (Geom * 2)(), C.c_size_t(0)
        f = _fmt()
        rc = L.ccmi_latents_render_blend_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(bad),
                                              None, geom, None, None, C.byref(need))
        _is_arg_error(rc, 1, "term 1", "weight")
        assert need.value == 0
        rc = L.ccmi_latents_render_blend_plan(H.h, idx, 2, None, 0, 444, C.byref(f), None, None, None, None, None,
                                              C.byref(good), None, geom, None, None, C.byref(need))
        _is_arg_error(rc, 0, "term 1", "source 1")  # frames 2 and 0 of the handle: a Kodak frame and a class D one
        assert need.value == 0
        op, cp = (C.c_void_p * 2)(FAKE, 0), (C.c_size_t * 2)(1 << 30, 0)
        rc = L.ccmi_latents_render_blend(H.h, idx, 2, None, op, cp, C.byref(f), None, None, None, None, None, C.byref(good),
                                         None, 0, 444, None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


def test_every_error_from_a_plan_only_handle(L, data):
    """The list of ccmi.h once more through ccmi_latents_render_blend_plan: frames 0, 0, 1 of the handle at one
    stored size, then whole frames of two sizes.  (The run entry point refuses a plan-only handle before it plans.)"""
    import ccmi
    n = 3
    good = [[(0, 0.5), (1, 0.5)], [(1, 1.0)], [(2, 0.25), (0, 0.75)]]
    cases = []
    for bad in (-1, 9):
        b, keep = _blend(n, terms=good)
        keep[0][1] = bad
        cases.append((b, keep, None, 1, ("blend terms", str(bad))))
    for member in ("source", "weight"):
        b, keep = _blend(n, terms=good)
        setattr(b, member, None)
        cases.append((b, keep, None, 0, ("blend", "NULL")))
    for bad in (-1, 3):
        b, keep = _blend(n, terms=[good[0], good[1], [(2, 0.25), (bad, 0.75)]])
        cases.append((b, keep, None, 2, ("term 1", "source", str(bad))))
    for bad in (NAN, INF):
        b, keep = _blend(n, terms=[good[0], [(1, bad)], good[2]])
        cases.append((b, keep, None, 1, ("term 0", "weight", "finite")))
    b, keep = _blend(n, terms=good, silent=[0, 0, 1])
    cases.append((b, keep, None, 2, ("silent", "terms")))
    b, keep = _blend(n, terms=[good[0], good[1], []], silent=[0, 0, 1])
    m, keepm = _mix(n, erase=[[], [], [R0]])
    cases.append((b, (keep, keepm), m, 2, ("silent", "rectangles")))
    m2, keepm2 = _mix(n, partner=[-1, -1, 0], lam=[0.5] * n)
    cases.append((b, (keep, keepm2), m2, 2, ("silent", "partner")))
    with Handle(L, data) as H:
        idx = (C.c_int * n)(0, 0, 1)
        rects = _rects([(16, 8, 21, 37)] * n, n)
        geom, need = (Geom * n)(), C.c_size_t(0)
        f = _fmt()
        for b, keep, m, frame, words in cases:
            rc = L.ccmi_latents_render_blend_plan(H.h, idx, n, rects, 0, 444, C.byref(f), None, None, None, None, None, C.byref(b),
                                                  _ref(m), geom, None, None, C.byref(need))
            _is_arg_error(rc, frame, *words)
            assert need.value == 0
        # blend without a format; a source of another stored size (whole frames of streams 0 and 1)
        b, keep = _blend(n, terms=good)
        rc = L.ccmi_latents_render_blend_plan(H.h, idx, n, rects, 0, 444, None, None, None, None, None, None, C.byref(b), None,
                                              geom, None, None, C.byref(need))
        _is_arg_error(rc, 0, "null")
        rc = L.ccmi_latents_render_blend_plan(H.h, idx, n, None, 0, 444, C.byref(f), None, None, None, None, None, C.byref(b), None,
                                              geom, None, None, C.byref(need))
        _is_arg_error(rc, 2, "term 1", "source 0", "416 x 240")
        assert need.value == 0
        # the valid ones plan, a silent frame's geometry included
        b, keep = _blend(n, terms=[good[0], good[1], []], silent=[0, 0, 1])
        assert L.ccmi_latents_render_blend_plan(H.h, idx, n, rects, 0, 444, C.byref(f), None, None, None, None, None, C.byref(b),
                                                None, geom, None, None, C.byref(need)) == 0, ccmi.last_error()
        assert need.value > 0 and [(g.width, g.height) for g in geom] == [(21, 37)] * n


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2, 1]
    m = len(index)
    rects = [(0, 0, 64, 48), (640, 360, 200, 100), (16, 8, 100, 60), (3, 5, 40, 40), (8, 8, 80, 80)]
    blend, keep = _blend(m, terms=[[(0, 0.5), (1, 0.25), (3, 0.25)], [], [], [], []], silent=[0, 1, 0, 1, 0])
    mix, keepm = _mix(m, erase=[[R0], [], [], [], []], partner=[2, -1, -1, -1, -1], lam=[0.5] * m)
    tone, keept = _tone([[(T_EQUALIZE, None)], [], [(T_SHARPNESS, 2.0)], [], []])
    flt, keepf = _filter([[0.5, 0.25], [], [], [], []], [2.0, 2.0, 2.0, 2.0, 2.0])
    f = _fmt(E_F32)
    rs = Rs(32, 24, 0)
    with Handle(L, data) as H:
        idx = (C.c_int * m)(*index)
        geom, info, need = (Geom * m)(), (Info * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_blend_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              C.byref(tone), C.byref(flt), C.byref(blend), C.byref(mix), geom, info, None,
                                              C.byref(need))
        assert rc == 0, ccmi.last_error()
        got = _plan(L, [data[i] for i in index], f, blend, mix, tone, flt, rects=rects, rs=rs)
        assert got[0] == 0, ccmi.last_error()
        for a, b in zip(geom, got[1]):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (32, 24)
        # the base: the _mix call that stages frames 0 .. 3 (0 by its rectangle, 2 as 0's partner, 1 and 3 as their own)
        bmix, keepx = _mix(m, erase=[[R0], [], [], [], []], partner=[2, 1, -1, 3, -1], lam=[0.5, 1.0, 0.5, 1.0, 0.5])
        n0 = C.c_size_t(0)
        assert L.ccmi_latents_render_mix_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                              C.byref(tone), C.byref(flt), C.byref(bmix), geom, None, None, C.byref(n0)) == 0
        assert need.value - n0.value == 256
        n1 = C.c_size_t(0)
        assert L.ccmi_latents_render_blend_plan(H.h, idx, m, _rects(rects, m), 0, 444, C.byref(f), C.byref(rs), None, None,
                                                C.byref(tone), C.byref(flt), None, C.byref(bmix), geom, None, None,
                                                C.byref(n1)) == 0
        assert n1.value == n0.value
