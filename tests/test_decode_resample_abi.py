"""ccmi_decode_batch_dev_rs(_plan) / ccmi_latents_render_rs(_plan): the host side of the
resampled formatted output (ccmi_resample).  As tests/test_decode_fmt_abi.py: no compute here,
the plan calls make no GPU call, the latent handles are plan-only, and the run entry point is
only ever called with arguments the plan rejects (made-up device pointers that nothing
dereferences)."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
COOL = ROOT / "tests" / "golden" / "cool"
E_F32, E_F16, E_BF16 = 0, 1, 2
ERR_ARG = 1
MAX_GRIDS = 8
P, I, Z = C.c_void_p, C.c_int, C.c_size_t
FAKE = 0x7F0000000000


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


class Rs(C.Structure):
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("filter", C.c_int)]


def _fmt(elem=E_F32, strides=(0, 0, 0)):
    f = Fmt(elem=elem, colour=1)
    for c in range(3):
        f.scale[c], f.bias[c] = 1.0, 0.0
    f.stride_c, f.stride_y, f.stride_x = strides
    return f


def _first(prefix):
    return sorted(COOL.rglob(prefix + "*.cool"))[0].read_bytes()


@pytest.fixture(scope="module")
def data():
    """class D 416 x 240 and class E 1280 x 720 (yuv420), a Kodak stream (rgb)"""
    return [_first("D-"), _first("E-"), _first("kodim")]


def _args(data):
    n = len(data)
    bufs = [C.create_string_buffer(d, len(d)) for d in data]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
    ln = (C.c_size_t * n)(*[len(d) for d in data])
    return bufs, sp, ln


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    lib.ccmi_decode_batch_dev_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_decode_batch_dev_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
    lib.ccmi_decode_batch_dev_rs.argtypes = [P, P, I, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_latents_render_fmt_plan.argtypes = [P, P, I, P, I, I, P, P, P, P]
    lib.ccmi_latents_render_rs_plan.argtypes = [P, P, I, P, I, I, P, P, P, P, P]
    lib.ccmi_latents_render_rs.argtypes = [P, P, I, P, P, P, P, P, I, I, P, Z, P]
    lib.ccmi_decode_last_tail_groups.argtypes = [P, P]
    for f in (lib.ccmi_decode_batch_dev_fmt_plan, lib.ccmi_decode_batch_dev_rs_plan, lib.ccmi_decode_batch_dev_rs,
              lib.ccmi_latents_decode, lib.ccmi_latents_render_fmt_plan, lib.ccmi_latents_render_rs_plan,
              lib.ccmi_latents_render_rs, lib.ccmi_decode_last_tail_groups):
        f.restype = C.c_int
    return lib


def _rects(rects, n):
    return None if rects is None else (Rect * n)(*[Rect(*r) for r in rects])


def _plan(lib, data, rects, fmt, rs, bitdepth=0, chroma=0):
    """(rc, geom, info, workspace bytes) of ccmi_decode_batch_dev_rs_plan; rs None: NULL"""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_rs_plan(sp, ln, n, _rects(rects, n), bitdepth, chroma, C.byref(fmt),
                                           None if rs is None else C.byref(rs), geom, info, C.byref(need))
    return rc, geom, info, need.value


def _plan_fmt(lib, data, rects, fmt, bitdepth=0, chroma=0):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    rc = lib.ccmi_decode_batch_dev_fmt_plan(sp, ln, n, _rects(rects, n), bitdepth, chroma, C.byref(fmt), geom, info,
                                            C.byref(need))
    return rc, geom, info, need.value


def _run(lib, data, rects, fmt, rs, caps, chroma=0):
    """ccmi_decode_batch_dev_rs with made-up device pointers: only for calls the plan rejects"""
    n = len(data)
    keep, sp, ln = _args(data)
    op = (C.c_void_p * n)(*[FAKE + (i << 32) for i in range(n)])
    cp = (C.c_size_t * n)(*caps)
    return lib.ccmi_decode_batch_dev_rs(sp, ln, n, _rects(rects, n), op, cp, C.byref(fmt), C.byref(rs), 0, chroma, None, 0,
                                        None)


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


def _fields(g):
    return [getattr(g, k) for k, _ in Geom._fields_]


def test_null_resample_is_the_fmt_plan(L, data):
    """rs = NULL: the geometry, the region info and the workspace of ccmi_decode_batch_dev_fmt_plan."""
    import ccmi
    for rects, chroma in ((None, 444), ([(352, 176, 64, 64), (1024, 464, 256, 256), (1, 3, 255, 77)], 0)):
        for elem in (E_F32, E_BF16):
            a = _plan(L, data, rects, _fmt(elem), None, chroma=chroma)
            b = _plan_fmt(L, data, rects, _fmt(elem), chroma=chroma)
            assert a[0] == 0 and b[0] == 0, ccmi.last_error()
            assert a[3] == b[3] and a[3] > 0
            for x, y in zip(a[1], b[1]):
                assert _fields(x) == _fields(y)
            for x, y in zip(a[2], b[2]):
                assert list(x.arm_rows) == list(y.arm_rows) and (x.windowed, x.n_grids) == (y.windowed, y.n_grids)


def test_geometry_follows_the_output_size(L, data):
    """Regions of three sizes, one output size: width / height / elems are the output's, chroma and
    bitdepth those the samples are taken at, ccmi_roi_info that of the same regions without a
    resample, and the workspace grows by at least the [3][h][out_w] float32 intermediates."""
    import ccmi
    rects = [(352, 176, 64, 32), (1024, 464, 256, 200), (1, 3, 255, 77)]
    for (ow, oh), chroma in (((224, 224), 0), ((7, 5), 444), ((300, 1), 0)):
        rc, geom, info, need = _plan(L, data, rects, _fmt(E_F16), Rs(ow, oh, 0), chroma=chroma)
        assert rc == 0, ccmi.last_error()
        rc, g0, i0, need0 = _plan_fmt(L, data, rects, _fmt(E_F16), chroma=chroma)
        assert rc == 0, ccmi.last_error()
        for g, b, fdt in zip(geom, g0, (1, 1, 0)):
            assert (g.width, g.height, g.elems) == (ow, oh, 3 * ow * oh)
            assert (g.bitdepth, g.chroma, g.frame_data_type) == (b.bitdepth, b.chroma, fdt)
        for a, b in zip(info, i0):
            assert list(a.arm_rows) == list(b.arm_rows) and (a.windowed, a.n_grids) == (b.windowed, b.n_grids)
        tmp = sum(3 * r[3] * ow * 4 for r in rects)
        assert need0 + tmp <= need <= need0 + tmp + 3 * 256 + 3 * 64


def test_render_plan_matches_the_decode_plan(L, data):
    import ccmi
    index = [1, 1, 0, 2]
    rects = [(0, 0, 256, 256), (1024, 464, 100, 256), (352, 176, 64, 64), (2, 2, 10, 6)]
    with Handle(L, data) as H:
        m = len(index)
        idx, arr = (C.c_int * m)(*index), _rects(rects, m)
        f, rs = _fmt(E_BF16), Rs(96, 64, 0)
        geom, need = (Geom * m)(), C.c_size_t(0)
        rc = L.ccmi_latents_render_rs_plan(H.h, idx, m, arr, 0, 0, C.byref(f), C.byref(rs), geom, None, C.byref(need))
        assert rc == 0, ccmi.last_error()
        rc, gd, _, _ = _plan(L, [data[i] for i in index], rects, f, rs)
        assert rc == 0, ccmi.last_error()
        for a, b in zip(geom, gd):
            assert _fields(a) == _fields(b) and (a.width, a.height) == (96, 64)
        # rs = NULL: the _fmt render plan
        g1, n1, g2, n2 = (Geom * m)(), C.c_size_t(0), (Geom * m)(), C.c_size_t(0)
        assert L.ccmi_latents_render_rs_plan(H.h, idx, m, arr, 0, 0, C.byref(f), None, g1, None, C.byref(n1)) == 0
        assert L.ccmi_latents_render_fmt_plan(H.h, idx, m, arr, 0, 0, C.byref(f), g2, None, C.byref(n2)) == 0
        assert n1.value == n2.value < need.value
        assert [_fields(g) for g in g1] == [_fields(g) for g in g2]
        # errors name the output frame; a plan-only handle cannot render
        bad = Rs(96, 0, 0)
        rc = L.ccmi_latents_render_rs_plan(H.h, idx, m, arr, 0, 0, C.byref(f), C.byref(bad), geom, None, C.byref(need))
        _is_arg_error(rc, 0, "output size")
        op, cp = (C.c_void_p * m)(*[FAKE] * m), (C.c_size_t * m)(*[1 << 30] * m)
        rc = L.ccmi_latents_render_rs(H.h, idx, m, arr, op, cp, C.byref(f), C.byref(rs), 0, 0, None, 0, None)
        assert rc == ERR_ARG and "plan-only" in ccmi.last_error()


@pytest.mark.parametrize("ow,oh", ((0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385), (1 << 30, 1 << 30)))
def test_output_size_outside_the_range(L, data, ow, oh):
    rc, _, _, got = _plan(L, data[:2], [(0, 0, 64, 64)] * 2, _fmt(), Rs(ow, oh, 0))
    _is_arg_error(rc, 0, "output size", "16384")
    assert got == 0  # nothing planned: the workspace size is not even written
    rc = _run(L, data[:2], [(0, 0, 64, 64)] * 2, _fmt(), Rs(ow, oh, 0), [1 << 30] * 2)
    _is_arg_error(rc, 0, "output size")


def test_output_size_at_the_limits_is_accepted(L, data):
    import ccmi
    for ow, oh in ((1, 1), (16384, 1), (1, 16384)):
        rc, geom, _, _ = _plan(L, data[:1], [(0, 0, 64, 64)], _fmt(), Rs(ow, oh, 0))
        assert rc == 0, ccmi.last_error()
        assert (geom[0].width, geom[0].height) == (ow, oh)


def test_unknown_filter(L, data):
    for filt in (1, -1, 77):
        rc, _, _, got = _plan(L, data[:2], None, _fmt(), Rs(32, 32, filt), chroma=444)
        _is_arg_error(rc, 0, "filter")
        assert got == 0
        rc = _run(L, data[:2], None, _fmt(), Rs(32, 32, filt), [1 << 30] * 2, chroma=444)
        _is_arg_error(rc, 0, "filter")


def _header_only(h, w):
    """A stream that is a valid header pass of an h x w frame: a committed stream's bytes with the
    GOP header's size rewritten (a plan reads the headers and the substream sizes only)."""
    b = bytearray(_first("D-"))
    b[2:4], b[4:6] = h.to_bytes(2, "big"), w.to_bytes(2, "big")
    return bytes(b)


def test_region_side_above_the_limit(L):
    """A frame 20000 wide: a region 16385 wide (or the whole frame) is refused, 16384 is taken."""
    import ccmi
    wide = [_header_only(64, 20000), _header_only(64, 20000)]
    ok = (0, 0, 16384, 64)
    rc, geom, _, need = _plan(L, wide, [ok, ok], _fmt(), Rs(224, 224, 0))
    assert rc == 0, ccmi.last_error()
    assert (geom[1].width, geom[1].height) == (224, 224)
    for bad in ((0, 0, 16386, 64), (2, 0, 19998, 64)):
        rc, _, _, got = _plan(L, wide, [ok, bad], _fmt(), Rs(224, 224, 0))
        _is_arg_error(rc, 1, "16384", "region")
        assert got == 0
    rc, *_ = _plan(L, wide, None, _fmt(), Rs(224, 224, 0))
    _is_arg_error(rc, 0, "16384", "region")
    tall = [_header_only(20000, 64)]
    rc, *_ = _plan(L, tall, [(0, 0, 64, 16386)], _fmt(), Rs(8, 8, 0))
    _is_arg_error(rc, 0, "16384", "region")
    # without a resample the same regions plan as ever
    rc, *_ = _plan(L, wide, [ok, (0, 0, 16386, 64)], _fmt(), None)
    assert rc == 0, ccmi.last_error()


def test_420_evenness_is_on_the_region_only(L, data):
    import ccmi
    d = [data[0], data[0]]
    ok = (0, 0, 64, 64)
    for ow, oh in ((7, 5), (1, 1), (33, 64)):  # odd output sizes at 420
        rc, geom, _, _ = _plan(L, d, [ok, (2, 4, 10, 6)], _fmt(), Rs(ow, oh, 0))
        assert rc == 0, ccmi.last_error()
        assert (geom[1].width, geom[1].height, geom[1].chroma) == (ow, oh, 420)
    for bad in ((0, 0, 63, 64), (0, 0, 64, 63)):
        rc, *_ = _plan(L, d, [ok, bad], _fmt(), Rs(8, 8, 0))
        _is_arg_error(rc, 1, "even", "444")
    rc, *_ = _plan(L, d, [ok, (1, 0, 64, 64)], _fmt(), Rs(8, 8, 0))
    _is_arg_error(rc, 1, "even origin")
    rc, geom, _, _ = _plan(L, d, [ok, (1, 3, 5, 7)], _fmt(), Rs(8, 8, 0), chroma=444)
    assert rc == 0, ccmi.last_error()


def test_capacity_and_aliasing_use_the_output_size(L, data):
    """out_caps and the stride-aliasing rule refer to the out_h x out_w frame, not to the region."""
    d = [data[0], data[0]]
    rects = [(0, 0, 64, 32), (16, 8, 8, 4)]
    ow, oh = 10, 6
    rs = Rs(ow, oh, 0)
    for elem, size in ((E_F32, 4), (E_F16, 2)):
        for strides in ((0, 0, 0), (1, 3 * ow, 3), (40 * 80, 80, 1)):
            sc, sy, sx = strides if any(strides) else (ow * oh, ow, 1)
            need = (2 * sc + (oh - 1) * sy + (ow - 1) * sx + 1) * size
            f = _fmt(elem, strides)
            rc = _run(L, d, rects, f, rs, [need, need - 1])
            _is_arg_error(rc, 1, str(need), str(need - 1))
            rc = _run(L, d, rects, f, rs, [need - size, need])
            _is_arg_error(rc, 0, str(need))
    import ccmi
    # contiguous strides of the OUTPUT frame pass; those of the first region (64 x 32) leave gaps and
    # pass too; strides that fit the small second region (8 x 4) but not the output alias
    for strides in ((ow * oh, ow, 1), (64 * 32, 64, 1)):
        rc, *_ = _plan(L, d, rects, _fmt(strides=strides), rs)
        assert rc == 0, (strides, ccmi.last_error())
    rc, *_ = _plan(L, d, rects, _fmt(strides=(32, 8, 1)), rs)
    _is_arg_error(rc, 0, "alias")


def test_null_arguments_and_the_group_counters(L, data):
    import ccmi
    keep, sp, ln = _args(data)
    geom, need = (Geom * 3)(), C.c_size_t(0)
    f, rs = _fmt(), Rs(8, 8, 0)
    assert L.ccmi_decode_batch_dev_rs_plan(sp, ln, 3, None, 0, 0, None, C.byref(rs), geom, None, C.byref(need)) == ERR_ARG
    assert L.ccmi_decode_batch_dev_rs_plan(sp, ln, 3, None, 0, 0, C.byref(f), C.byref(rs), None, None, C.byref(need)) == ERR_ARG
    assert L.ccmi_decode_batch_dev_rs(sp, ln, 3, None, None, None, C.byref(f), C.byref(rs), 0, 0, None, 0, None) == ERR_ARG
    assert "null" in ccmi.last_error()
    a, b = C.c_int(7), C.c_int(7)
    assert L.ccmi_decode_last_tail_groups(None, C.byref(b)) == ERR_ARG
    # a call that only plans reports no launches
    assert L.ccmi_decode_batch_dev_rs_plan(sp, ln, 3, None, 0, 444, C.byref(f), C.byref(rs), geom, None, C.byref(need)) == 0
    assert L.ccmi_decode_last_tail_groups(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
