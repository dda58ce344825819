"""ccmi_decode_batch_dev_roi_plan: the header-only pass of the region decode
(ccmi_decode_batch_dev_roi).  No compute here (CPU hosts have no HIP device): the whole-frame
case against ccmi_decode_batch_dev_plan, the region's geometry, the argument errors, the rows
the ARM decode will produce against the level recurrence restated below, and the workspace."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
COOL = ROOT / "tests" / "golden" / "cool"
FILES = sorted(COOL.rglob("*.cool"))
U8, U16, F32 = 0, 1, 2
MAX_GRIDS = 8


class Geom(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bitdepth", C.c_int), ("chroma", C.c_int),
                ("frame_data_type", C.c_int), ("elems", C.c_size_t)]


class Rect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class Info(C.Structure):
    _fields_ = [("n_grids", C.c_int), ("arm_rows", C.c_int * MAX_GRIDS), ("windowed", C.c_int)]


def _args(data):
    n = len(data)
    bufs = [C.create_string_buffer(d, len(d)) for d in data]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
    ln = (C.c_size_t * n)(*[len(d) for d in data])
    return bufs, sp, ln


def _plans(lib):
    f = lib.ccmi_decode_batch_dev_plan
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    g = lib.ccmi_decode_batch_dev_roi_plan
    g.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                  C.c_void_p]
    g.restype = C.c_int
    return f, g


def _roi_plan(lib, data, rects, bitdepth=0, chroma=0, sample=U16):
    """(rc, geom, info, workspace bytes) of one region plan call."""
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    arr = None if rects is None else (Rect * n)(*[Rect(*r) for r in rects])
    rc = _plans(lib)[1](sp, ln, n, arr, bitdepth, chroma, sample, geom, info, C.byref(need))
    return rc, geom, info, need.value


def test_whole_frame_region_is_the_whole_frame_plan(ccmi_lib):
    """roi NULL and roi (0, 0, W, H): the geometry and workspace_bytes of
    ccmi_decode_batch_dev_plan, for every committed stream, and every latent row is decoded."""
    import ccmi
    assert len(FILES) > 30
    plan = _plans(ccmi_lib)[0]
    for f in FILES:
        data = [f.read_bytes()]
        keep, sp, ln = _args(data)
        g0, need0 = (Geom * 1)(), C.c_size_t(0)
        assert plan(sp, ln, 1, 0, 0, U16, g0, C.byref(need0)) == 0, ccmi.last_error()
        full = (0, 0, g0[0].width, g0[0].height)
        for rects in (None, [full]):
            rc, g, info, need = _roi_plan(ccmi_lib, data, rects)
            assert rc == 0, ccmi.last_error()
            assert need == need0.value, (f.name, rects)
            assert [getattr(g[0], k) for k, _ in Geom._fields_] == [getattr(g0[0], k) for k, _ in Geom._fields_], f.name
            hh = g0[0].height
            for l in range(info[0].n_grids):
                assert info[0].arm_rows[l] == hh, (f.name, l)
                hh = (hh + 1) // 2
    # a batch: the sum is the batch's plan too
    data = [f.read_bytes() for f in FILES[:7]]
    keep, sp, ln = _args(data)
    g0, need0 = (Geom * 7)(), C.c_size_t(0)
    assert plan(sp, ln, 7, 0, 0, U16, g0, C.byref(need0)) == 0, ccmi.last_error()
    rc, g, info, need = _roi_plan(ccmi_lib, data, None)
    assert rc == 0 and need == need0.value


def test_region_geometry_and_errors(ccmi_lib):
    import ccmi
    data = [(COOL / "D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool").read_bytes()]
    W, H = 416, 240
    rc, g, info, need = _roi_plan(ccmi_lib, data, [(3, 5, 65, 33)], chroma=444)
    assert rc == 0, ccmi.last_error()
    assert (g[0].width, g[0].height, g[0].chroma, g[0].elems) == (65, 33, 444, 3 * 65 * 33)
    rc, g, info, need = _roi_plan(ccmi_lib, data, [(2, 4, 65, 33)], chroma=420)
    assert rc == 0, ccmi.last_error()
    assert (g[0].width, g[0].height, g[0].chroma, g[0].elems) == (65, 33, 420, 65 * 33 + 2 * 16 * 32)
    rc, g, info, need = _roi_plan(ccmi_lib, data, [(0, 0, 1, 1)], chroma=420)
    assert rc == 0 and g[0].elems == 1, ccmi.last_error()
    for what, r, chroma in (
        ("odd x at 420", (3, 4, 16, 16), 420),
        ("odd y at 420", (2, 5, 16, 16), 420),
        ("w = 0", (0, 0, 0, 16), 444),
        ("h = 0", (0, 0, 16, 0), 444),
        ("x + w = W + 1", (W - 15, 0, 16, 16), 444),
        ("y + h = H + 1", (0, H - 15, 16, 16), 444),
        ("negative x", (-2, 0, 16, 16), 444),
        ("negative y", (0, -2, 16, 16), 444),
        ("overflowing x + w", (2, 0, 2**31 - 1, 16), 444),
    ):
        rc, g, info, need = _roi_plan(ccmi_lib, data, [r], chroma=chroma)
        assert rc == ccmi.ERR_ARG, what
        assert "stream 0" in ccmi.last_error(), (what, ccmi.last_error())
    # an odd origin is fine at 444
    assert _roi_plan(ccmi_lib, data, [(3, 5, 16, 16)], chroma=444)[0] == 0
    # the message names the stream at fault
    rc, g, info, need = _roi_plan(ccmi_lib, data * 3, [(0, 0, 16, 16), (0, 0, 16, 16), (W, 0, 16, 16)], chroma=444)
    assert rc == ccmi.ERR_ARG and "stream 2" in ccmi.last_error()
    # the decode entry point rejects the same regions from the headers alone (no HIP call)
    dec = ccmi_lib.ccmi_decode_batch_dev_roi
    dec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                    C.c_void_p, C.c_size_t, C.c_void_p]
    dec.restype = C.c_int
    keep, sp, ln = _args(data)
    out = (C.c_void_p * 1)(0x1000)  # never dereferenced: every call below fails its checks first
    cap = (C.c_size_t * 1)(2 * 3 * 16 * 16)
    short = (C.c_size_t * 1)(2 * 3 * 16 * 16 - 1)
    ok_rect, bad_rect = (Rect * 1)(Rect(0, 0, 16, 16)), (Rect * 1)(Rect(W - 15, 0, 16, 16))
    assert dec(sp, ln, 1, bad_rect, out, cap, U16, 0, 444, None, 0, None) == ccmi.ERR_ARG
    assert dec(sp, ln, 1, ok_rect, out, short, U16, 0, 444, None, 0, None) == ccmi.ERR_ARG
    assert dec(sp, ln, 1, ok_rect, None, cap, U16, 0, 444, None, 0, None) == ccmi.ERR_ARG


def _expected_arm_rows(desc, rect):
    """The level recurrence, restated from the kernels' taps.  rect = (x, y, w, h).

    Level 0 (the synthesis input): the rect grown by the sum of (ks - 1) / 2 over the synthesis
    layers, clipped to the frame.  A pyramid step's destination row Y reads source rows
    (Y >> 1) - pad + (Y & 1) .. that + taps - 1, with taps = ups_k / 2 per phase and pad =
    taps / 2 (8-tap kernels: the last row read is (Y >> 1) + (Y & 1) + 1), clamped to the plane.
    The refined channel of a level reads its latent grid pre_k / 2 rows either side.  The ARM
    decode of grid l produces the rows above the bottom of what is read from it."""
    L = desc.n_grids
    hs = [desc.h]
    for _ in range(1, L):
        hs.append((hs[-1] + 1) // 2)
    n_sp = sum((k - 1) // 2 for k in desc.syn_ks[: desc.n_syn_layers])
    taps = desc.ups_k // 2
    pad = taps // 2
    x, y, w, h = rect
    bottom = [min(hs[0], y + h + n_sp)]
    for k in range(1, L):
        b = bottom[-1]
        bottom.append(min(hs[k], ((b - 1) >> 1) + ((b - 1) & 1) - pad + taps))
    return [bottom[l] if l == L - 1 else min(hs[l], bottom[l] + desc.pre_k // 2) for l in range(L)], n_sp


@pytest.mark.parametrize("name", ["D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool",
                                  "E-Johnny-lmbda-0004_1280x720_60p_yuv420_8b.cool",
                                  "B-BQTerrace-lmbda-0001_1920x1080_50p_yuv420_8b.cool"])
def test_arm_rows_follow_the_level_recurrence(ccmi_lib, name):
    import ccmi
    from ccmi import encode
    data = [(COOL / name).read_bytes()]
    desc = encode.parse(data[0]).desc
    assert (desc.ups_k, desc.pre_k) == (8, 7)
    W, H = desc.w, desc.h
    rects = [(0, 0, 64, 64), (W - 64, H - 64, 64, 64), (0, 0, W, 1), (0, 0, 416, 8)]
    if W >= 256 and H >= 256:
        rects.append((((W - 256) // 2) & ~1, ((H - 256) // 2) & ~1, 256, 256))
    for r in rects:
        rc, g, info, need = _roi_plan(ccmi_lib, data, [r])
        assert rc == 0, ccmi.last_error()
        want, n_sp = _expected_arm_rows(desc, r)
        got = list(info[0].arm_rows[: info[0].n_grids])
        assert info[0].n_grids == desc.n_grids and info[0].windowed == 1
        assert got == want, (name, r, got, want)
        hh = H
        for l in range(desc.n_grids):
            assert 1 <= got[l] <= hh
            hh = (hh + 1) // 2
        if r == (0, 0, 416, 8):
            assert got[0] == 8 + n_sp + 3, (got, n_sp)
        if r[1] + r[3] == H:  # a region that touches the last row needs every latent row
            want_full, hh = [], H
            for l in range(desc.n_grids):
                want_full.append(hh)
                hh = (hh + 1) // 2
            assert got == want_full


def test_region_workspace_is_sized_by_the_window(ccmi_lib):
    import ccmi
    data = [(COOL / "B-BQTerrace-lmbda-0001_1920x1080_50p_yuv420_8b.cool").read_bytes()]
    rc, g, info, full = _roi_plan(ccmi_lib, data, None)
    assert rc == 0, ccmi.last_error()
    rc, g, info, small = _roi_plan(ccmi_lib, data, [(928, 508, 64, 64)])
    assert rc == 0, ccmi.last_error()
    assert small < full, f"64x64 region of 1080p: {small} workspace bytes, whole frame: {full}"
    # the top-left region decodes few latent rows, so its latent planes are small too
    rc, g, info, top = _roi_plan(ccmi_lib, data, [(0, 0, 64, 64)])
    assert rc == 0 and top < small, f"top-left 64x64: {top} bytes, centred 64x64: {small} bytes"
    print(f"1080p workspace bytes: whole frame {full}, centred 64x64 {small}, top-left 64x64 {top}")


def test_python_roi_plan_and_geometry(ccmi_lib):
    from ccmi import decode, encode
    name = "D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool"
    data = [(COOL / name).read_bytes()] * 2
    desc = encode.parse(data[0]).desc
    geom, need = decode.decode_batch_geometry(data, roi=[(0, 0, 64, 32), None])
    assert [(g["width"], g["height"]) for g in geom] == [(64, 32), (416, 240)]
    geom1, need1 = decode.decode_batch_geometry(data, roi=(0, 0, 64, 32))
    assert [(g["width"], g["height"]) for g in geom1] == [(64, 32)] * 2 and need1 < need
    plan = decode.roi_plan(data, [(0, 0, 64, 32), None])
    assert plan[0]["arm_rows"] == _expected_arm_rows(desc, (0, 0, 64, 32))[0] and plan[0]["windowed"] is True
    assert plan[1]["arm_rows"][0] == 240
    with pytest.raises(ValueError):
        decode.roi_plan(data, [(0, 0, 64, 32)])
    with pytest.raises(decode.CcmiError):
        decode.roi_plan(data, (0, 0, 417, 32))
