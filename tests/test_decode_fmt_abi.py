"""ccmi_decode_batch_dev_fmt(_plan) / ccmi_latents_render_fmt(_plan): the host side of the
formatted output (ccmi_tensor_fmt).  No compute here (CPU hosts have no HIP device): the plan
calls make no GPU call, the latent handles are plan-only, and the run entry point is only ever
called with arguments the plan rejects, which it does before any GPU work (the device pointers
are made-up addresses that nothing dereferences).  Geometry, the workspace size against the
CCMI_SAMPLE_F32 plan of the same call, and every argument error of the contract in ccmi.h."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
COOL = ROOT / "tests" / "golden" / "cool"
F32 = 2                      # CCMI_SAMPLE_F32
E_F32, E_F16, E_BF16 = 0, 1, 2
ASIS, RGB = 0, 1
ERR_ARG = 1
MAX_GRIDS = 8
P, I, Z = C.c_void_p, C.c_int, C.c_size_t
FAKE = 0x7F0000000000        # a "device pointer" for calls the plan rejects; 256-byte aligned


class Geom(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bitdepth", C.c_int), ("chroma", C.c_int),
                ("frame_data_type", C.c_int), ("elems", C.c_size_t)]


class Rect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class Info(C.Structure):
    _fields_ = [("n_grids", C.c_int), ("arm_rows", C.c_int * MAX_GRIDS), ("windowed", C.c_int)]


class Fmt(C.Structure):
    _fields_ = [("elem", C.c_int), ("colour", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3),
                ("stride_c", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("mirror", C.c_void_p)]


def _fmt(elem=E_F32, colour=RGB, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), strides=(0, 0, 0)):
    f = Fmt(elem=elem, colour=colour)
    for c in range(3):
        f.scale[c], f.bias[c] = scale[c], bias[c]
    f.stride_c, f.stride_y, f.stride_x = strides
    return f


def _first(prefix):
    return sorted(COOL.rglob(prefix + "*.cool"))[0].read_bytes()


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


def _sizes(data):
    """(width, height, frame_data_type) per stream: the GOP header's size, yuv420 for classes D and E"""
    return [(int.from_bytes(d[4:6], "big"), int.from_bytes(d[2:4], "big"), 1 if i < 2 else 0) for i, d in enumerate(data)]


def _args(data):
    n = len(data)
    bufs = [C.create_string_buffer(d, len(d)) for d in data]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
    ln = (C.c_size_t * n)(*[len(d) for d in data])
    return bufs, sp, ln


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    lib.ccmi_decode_batch_dev_roi_plan.argtypes = [P, P, I, P, I, I, I, P, P, P]
    lib.ccmi_decode_batch_dev_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_decode_batch_dev_fmt.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_latents_render_plan.argtypes = [P, P, I, P, I, I, I, P, P, P]
    lib.ccmi_latents_render_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_latents_render_fmt.argtypes = [P, P, I, P, P, P, P, I, I, P, Z, P]
    for f in (lib.ccmi_decode_batch_dev_roi_plan, lib.ccmi_decode_batch_dev_fmt_plan, lib.ccmi_decode_batch_dev_fmt,
              lib.ccmi_latents_decode, lib.ccmi_latents_render_plan, lib.ccmi_latents_render_fmt_plan,
              lib.ccmi_latents_render_fmt):
        f.restype = C.c_int
    return lib


def _rects(rects, n):
    return None if rects is None else (Rect * n)(*[Rect(*r) for r in rects])


def _plan(lib, data, rects, fmt, bitdepth=0, chroma=0):
    """(rc, geom, info, workspace bytes) of ccmi_decode_batch_dev_fmt_plan"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_fmt_plan(sp, ln, n, _rects(rects, n), bitdepth, chroma, C.byref(fmt), geom, info,
                                            C.byref(need))
    return rc, geom, info, need.value


def _plan_f32(lib, data, rects, bitdepth=0, chroma=0):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_roi_plan(sp, ln, n, _rects(rects, n), bitdepth, chroma, F32, geom, info, C.byref(need))
    return rc, geom, info, need.value


def _run(lib, data, rects, fmt, caps, ptrs=None, bitdepth=0, chroma=0):
    """ccmi_decode_batch_dev_fmt with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*(ptrs or [FAKE + (i << 32) for i in range(n)]))
    cp = (C.c_size_t * n)(*caps)
    return lib.ccmi_decode_batch_dev_fmt(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), bitdepth, chroma, None, 0, None)


class Handle:
    """A plan-only latent handle (store = NULL: no GPU call)."""

    def __init__(self, lib, data):
        import ccmi
        self.lib, self.h = lib, C.c_void_p(None)
        keep, sp, ln = _args(data)
        rc = lib.ccmi_latents_decode(sp, ln, len(data), 1, None, 0, None, 0, None, C.byref(self.h))
        assert rc == 0 and self.h.value, ccmi.last_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.ccmi_latents_free(self.h)


def _is_arg_error(rc, frame, *words):
    import ccmi
    msg = ccmi.last_error()
    assert rc == ERR_ARG, (rc, msg)
    assert re.search(r"\b(frame|stream|output) %d\b" % frame, msg), msg
    for w in words:
        assert w in msg, msg


def test_whole_frame_geometry_and_workspace(L, data):
    """Whole frames at 444 and at the streams' own chroma: the region's size, elems = 3 w h, the
    chroma the samples are taken at, and exactly the CCMI_SAMPLE_F32 workspace."""
    import ccmi
    assert _sizes(data)[:2] == [(416, 240, 1), (1280, 720, 1)]
    for chroma in (444, 0):
        for elem in (E_F32, E_F16, E_BF16):
            rc, geom, info, need = _plan(L, data, None, _fmt(elem=elem), chroma=chroma)
            assert rc == 0, ccmi.last_error()
            rc, g32, i32, need32 = _plan_f32(L, data, None, chroma=chroma)
            assert rc == 0, ccmi.last_error()
            assert need == need32 and need > 0
            for g, r, (w, h, fdt) in zip(geom, g32, _sizes(data)):
                want_chroma = chroma or (420 if fdt == 1 else 444)
                assert (g.width, g.height, g.bitdepth, g.chroma, g.frame_data_type) == (w, h, 8, want_chroma, fdt)
                assert g.elems == 3 * w * h
                assert (r.width, r.height, r.chroma) == (w, h, want_chroma)
            for a, b in zip(info, i32):
                assert list(a.arm_rows) == list(b.arm_rows) and a.windowed == b.windowed and a.n_grids == b.n_grids


def test_region_geometry_and_workspace(L, data):
    import ccmi
    rects = [(352, 176, 64, 64), (1024, 464, 256, 256), (1, 3, 255, 77)]
    for bitdepth, chroma in ((0, 0), (10, 0), (8, 444)):
        rc, geom, info, need = _plan(L, data, rects, _fmt(elem=E_BF16), bitdepth=bitdepth, chroma=chroma)
        assert rc == 0, ccmi.last_error()
        rc, g32, i32, need32 = _plan_f32(L, data, rects, bitdepth=bitdepth, chroma=chroma)
        assert rc == 0, ccmi.last_error()
        assert need == need32
        for g, (x, y, w, h), (_, _, fdt) in zip(geom, rects, _sizes(data)):
            assert (g.width, g.height, g.elems) == (w, h, 3 * w * h)
            assert g.bitdepth == (bitdepth or 8)
            assert g.chroma == (chroma or (420 if fdt == 1 else 444))
        for a, b in zip(info, i32):
            assert list(a.arm_rows) == list(b.arm_rows) and a.windowed == b.windowed


def test_strides_do_not_change_the_plan(L, data):
    import ccmi
    d = data[:1]
    rect = [(0, 0, 64, 32)]
    base = _plan(L, d, rect, _fmt())
    assert base[0] == 0, ccmi.last_error()
    for strides in ((64 * 32, 64, 1), (1, 3 * 64, 3), (40 * 80, 80, 1), (1, 1000, 4), (2, 6 * 64, 6)):
        rc, geom, _, need = _plan(L, d, rect, _fmt(strides=strides))
        assert rc == 0, (strides, ccmi.last_error())
        assert need == base[3] and geom[0].elems == 3 * 64 * 32


def test_render_plan_matches_the_decode_plan(L, data):
    """ccmi_latents_render_fmt_plan against ccmi_decode_batch_dev_fmt_plan for the same frames, and
    its workspace against ccmi_latents_render_plan at CCMI_SAMPLE_F32."""
    import ccmi
    index = [1, 1, 0, 2]
    rects = [(0, 0, 256, 256), (1024, 464, 256, 256), (352, 176, 64, 64), (2, 2, 10, 6)]
    with Handle(L, data) as H:
        m = len(index)
        idx, arr = (C.c_int * m)(*index), _rects(rects, m)
        geom, need = (Geom * m)(), C.c_size_t(0)
        f = _fmt(elem=E_F16)
        rc = L.ccmi_latents_render_fmt_plan(H.h, idx, m, arr, 0, 0, C.byref(f), geom, None, C.byref(need))
        assert rc == 0, ccmi.last_error()
        g32, need32 = (Geom * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_plan(H.h, idx, m, arr, 0, 0, F32, g32, None, C.byref(need32))
        assert rc == 0, ccmi.last_error()
        assert need.value == need32.value
        rc, gd, _, _ = _plan(L, [data[i] for i in index], rects, f)
        assert rc == 0, ccmi.last_error()
        for a, b in zip(geom, gd):
            assert [getattr(a, k) for k, _ in Geom._fields_] == [getattr(b, k) for k, _ in Geom._fields_]
        # errors name the output frame
        odd = _rects([(0, 0, 256, 256), (0, 0, 256, 256), (0, 0, 64, 63), (0, 0, 4, 4)], m)
        rc = L.ccmi_latents_render_fmt_plan(H.h, idx, m, odd, 0, 0, C.byref(f), geom, None, C.byref(need))
        _is_arg_error(rc, 2, "444")
        bad = _fmt(elem=7)
        rc = L.ccmi_latents_render_fmt_plan(H.h, idx, m, arr, 0, 0, C.byref(bad), geom, None, C.byref(need))
        _is_arg_error(rc, 0, "element")
        # a plan-only handle cannot render
        op, cp = (C.c_void_p * m)(*[FAKE] * m), (C.c_size_t * m)(*[1 << 30] * m)
        rc = L.ccmi_latents_render_fmt(H.h, idx, m, arr, op, cp, C.byref(f), 0, 0, None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


def test_420_needs_an_even_size_444_takes_any(L, data):
    d = [data[0], data[0]]
    ok = (0, 0, 64, 64)
    for bad in ((0, 0, 63, 64), (0, 0, 64, 63), (2, 2, 1, 1)):
        rc, *_ = _plan(L, d, [ok, bad], _fmt())
        _is_arg_error(rc, 1, "even", "444")
    # the existing even-origin rule still comes first
    rc, *_ = _plan(L, d, [ok, (1, 0, 64, 64)], _fmt())
    _is_arg_error(rc, 1, "even origin")
    # the same rectangles at 444 on the 420 stream
    import ccmi
    for r in ((0, 0, 63, 64), (0, 0, 64, 63), (2, 2, 1, 1), (1, 3, 5, 7)):
        rc, geom, _, _ = _plan(L, d, [ok, r], _fmt(), chroma=444)
        assert rc == 0, ccmi.last_error()
        assert (geom[1].width, geom[1].height, geom[1].chroma, geom[1].elems) == (r[2], r[3], 444, 3 * r[2] * r[3])


def test_a_whole_odd_frame_at_420_is_rejected(L):
    """The 420 planes of an odd frame hold h / 2 rows: a formatted whole frame is refused too."""
    odd = []
    for f in sorted((COOL / "clic").glob("*.cool")):
        b = f.read_bytes()
        h, w = int.from_bytes(b[2:4], "big"), int.from_bytes(b[4:6], "big")
        if (h | w) & 1:
            odd.append(b)
    assert odd, "no committed CLIC stream with an odd size left"
    rc, *_ = _plan(L, odd[:1], None, _fmt(), chroma=420)
    _is_arg_error(rc, 0, "even", "444")
    import ccmi
    rc, *_ = _plan(L, odd[:1], None, _fmt(), chroma=444)
    assert rc == 0, ccmi.last_error()


def test_unknown_elem_colour_and_non_finite_affine(L, data):
    d = [data[0], data[2]]
    for bad in (_fmt(elem=3), _fmt(elem=-1)):
        rc, *_ = _plan(L, d, None, bad)
        _is_arg_error(rc, 0, "element")
    for bad in (_fmt(colour=2), _fmt(colour=-1)):
        rc, *_ = _plan(L, d, None, bad)
        _is_arg_error(rc, 0, "colour")
    for v in (math.inf, -math.inf, math.nan):
        for c in range(3):
            s = [1.0, 1.0, 1.0]
            s[c] = v
            rc, *_ = _plan(L, d, None, _fmt(scale=s))
            _is_arg_error(rc, 0, "finite")
            rc, *_ = _plan(L, d, None, _fmt(bias=s))
            _is_arg_error(rc, 0, "finite")


def test_negative_and_aliasing_strides(L, data):
    d = [data[0], data[0]]
    rects = [(0, 0, 8, 4), (0, 0, 8, 4)]
    for strides in ((-1, 8, 1), (32, -8, 1), (32, 8, -1)):
        rc, *_ = _plan(L, d, rects, _fmt(strides=strides))
        _is_arg_error(rc, 0, "stride")
    # w 8, h 4: sorted by stride, each must step over stride x extent of the one before
    for strides in ((1, 1, 1), (32, 7, 1), (31, 8, 1), (1, 24, 2), (1, 23, 3), (0, 8, 1), (32, 0, 1), (32, 8, 0),
                    (2, 8, 1), (32, 8, 8)):
        rc, *_ = _plan(L, d, rects, _fmt(strides=strides))
        _is_arg_error(rc, 0, "alias")
    import ccmi
    for strides in ((32, 8, 1), (1, 24, 3), (4, 12, 128), (8, 100, 1), (1000, 3, 12)):
        rc, *_ = _plan(L, d, rects, _fmt(strides=strides))
        assert rc == 0, (strides, ccmi.last_error())


def test_capacity_and_alignment(L, data):
    """out_caps[j] >= (2 stride_c + (h - 1) stride_y + (w - 1) stride_x + 1) sizeof(elem), out_dev[j]
    aligned to one element: rejected by the run call before any GPU work."""
    d = [data[0], data[0]]
    rects = [(0, 0, 8, 4), (16, 8, 8, 4)]
    for elem, size in ((E_F32, 4), (E_F16, 2), (E_BF16, 2)):
        for strides in ((0, 0, 0), (1, 24, 3), (40 * 80, 80, 1), (2, 100, 7)):
            sc, sy, sx = strides if any(strides) else (32, 8, 1)
            need = (2 * sc + 3 * sy + 7 * sx + 1) * size
            f = _fmt(elem=elem, strides=strides)
            rc = _run(L, d, rects, f, [need, need - 1])
            _is_arg_error(rc, 1, str(need), str(need - 1))
            rc = _run(L, d, rects, f, [need - size, need])
            _is_arg_error(rc, 0, str(need))
        rc = _run(L, d, rects, _fmt(elem=elem), [1 << 20, 1 << 20], ptrs=[FAKE, FAKE + (1 << 32) + size // 2])
        _is_arg_error(rc, 1, "aligned")
    # the same checks answer the plan-rejected errors through the run call too
    rc = _run(L, d, rects, _fmt(elem=9), [1 << 20, 1 << 20])
    _is_arg_error(rc, 0, "element")
    rc = _run(L, d, [(0, 0, 8, 4), (0, 0, 8, 3)], _fmt(), [1 << 20, 1 << 20])
    _is_arg_error(rc, 1, "even")


def test_null_arguments(L, data):
    import ccmi
    keep, sp, ln = _args(data)
    geom, need = (Geom * 3)(), C.c_size_t(0)
    f = _fmt()
    assert L.ccmi_decode_batch_dev_fmt_plan(sp, ln, 3, None, 0, 0, None, geom, None, C.byref(need)) == ERR_ARG
    assert L.ccmi_decode_batch_dev_fmt_plan(sp, ln, 3, None, 0, 0, C.byref(f), None, None, C.byref(need)) == ERR_ARG
    assert L.ccmi_decode_batch_dev_fmt(sp, ln, 3, None, None, None, C.byref(f), 0, 0, None, 0, None) == ERR_ARG
    assert "null" in ccmi.last_error()
