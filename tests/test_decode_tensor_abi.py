"""ccmi_decode_batch_dev_plan: the header-only pass of the device-tensor decode
(ccmi_decode_batch_dev).  No compute here (CPU hosts have no HIP device): geometry against
ccmi.encode.parse, sample counts against the byte path's own plan, and the argument errors."""
import ctypes as C
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FILES = sorted((ROOT / "tests" / "golden" / "cool").rglob("*.cool"))
U8, U16, F32 = 0, 1, 2


class Geom(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bitdepth", C.c_int), ("chroma", C.c_int),
                ("frame_data_type", C.c_int), ("elems", C.c_size_t)]


def _args(data):
    n = len(data)
    bufs = [C.create_string_buffer(d, len(d)) for d in data]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
    ln = (C.c_size_t * n)(*[len(d) for d in data])
    return bufs, sp, ln


def _plan(lib):
    f = lib.ccmi_decode_batch_dev_plan
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f


def test_dev_plan_geometry_of_every_committed_stream(ccmi_lib):
    """Width / height equal encode.parse's; elems * sample size equals the YUV payload size
    ccmi_decode_batch_plan(as_yuv=1) reports for the stream's own bitdepth and chroma format."""
    import ccmi
    from ccmi import encode
    assert len(FILES) > 30
    data = [f.read_bytes() for f in FILES]
    n = len(data)
    keep, sp, ln = _args(data)
    plan = _plan(ccmi_lib)
    byte_plan = ccmi_lib.ccmi_decode_batch_plan
    byte_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    byte_plan.restype = C.c_int
    sizes, need_b = (C.c_size_t * n)(), C.c_size_t(0)
    assert byte_plan(sp, ln, n, 0, 0, 1, sizes, C.byref(need_b)) == 0, ccmi.last_error()
    geom, need = (Geom * n)(), C.c_size_t(0)
    assert plan(sp, ln, n, 0, 0, U16, geom, C.byref(need)) == 0, ccmi.last_error()
    assert 0 < need.value <= need_b.value  # no output staging in the workspace
    for f, d, g, sz in zip(FILES, data, geom, sizes):
        desc = encode.parse(d).desc
        assert (g.width, g.height) == (desc.w, desc.h), f.name
        assert g.bitdepth == desc.bitdepth and g.frame_data_type == desc.frame_data_type, f.name
        assert g.chroma == (420 if desc.frame_data_type == 1 else 444), f.name
        assert g.elems == (desc.h * desc.w + 2 * (desc.h // 2) * (desc.w // 2) if g.chroma == 420 else 3 * desc.h * desc.w)
        assert g.elems * (1 if g.bitdepth <= 8 else 2) == int(sz), f.name
    # the sample type changes neither the sample count nor the geometry
    g8, gf = (Geom * n)(), (Geom * n)()
    if all(g.bitdepth <= 8 for g in geom):
        assert plan(sp, ln, n, 0, 0, U8, g8, C.byref(need)) == 0, ccmi.last_error()
        assert [x.elems for x in g8] == [x.elems for x in geom]
    assert plan(sp, ln, n, 10, 420, F32, gf, C.byref(need)) == 0, ccmi.last_error()
    for g, x in zip(geom, gf):
        assert (x.bitdepth, x.chroma) == (10, 420)
        assert x.elems == g.height * g.width + 2 * (g.height // 2) * (g.width // 2)
    # every PPM bitdepth is accepted, not only the .yuv writer's 8 / 10
    for bd in (1, 7, 12, 16):
        assert plan(sp, ln, 1, bd, 444, U16, gf, C.byref(need)) == 0, ccmi.last_error()
        assert gf[0].bitdepth == bd and gf[0].elems == 3 * geom[0].height * geom[0].width


def test_byte_path_plan_entry_points_agree(ccmi_lib):
    """One planner behind the byte path's three header-only entry points: for every committed
    stream ccmi_decode_batch_workspace_bytes and ccmi_decode_batch_plan report the same
    workspace and the latter's out_sizes[0] is ccmi_decode_output_size, for as_yuv 0 and 1;
    the two workspace sizes agree for a batch of the first 7 streams too."""
    import ccmi
    every = FILES + sorted((ROOT / "tests" / "golden" / "cool_synth").rglob("*.cool"))
    assert len(every) > len(FILES) > 30
    ws_bytes = ccmi_lib.ccmi_decode_batch_workspace_bytes
    ws_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    ws_bytes.restype = C.c_int
    byte_plan = ccmi_lib.ccmi_decode_batch_plan
    byte_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    byte_plan.restype = C.c_int
    out_size = ccmi_lib.ccmi_decode_output_size
    out_size.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out_size.restype = C.c_int
    data = [f.read_bytes() for f in every]
    for as_yuv in (0, 1):
        for batch in [[d] for d in data] + [data[:7]]:
            n = len(batch)
            keep, sp, ln = _args(batch)
            need_a, need_b, sizes, one = C.c_size_t(0), C.c_size_t(0), (C.c_size_t * n)(), C.c_size_t(0)
            assert ws_bytes(sp, ln, n, 0, 0, as_yuv, C.byref(need_a)) == 0, ccmi.last_error()
            assert byte_plan(sp, ln, n, 0, 0, as_yuv, sizes, C.byref(need_b)) == 0, ccmi.last_error()
            assert need_a.value == need_b.value > 0
            if n == 1:
                assert out_size(sp[0], ln[0], 0, 0, as_yuv, C.byref(one)) == 0, ccmi.last_error()
                assert sizes[0] == one.value > 0


def test_dev_plan_errors_are_reported(ccmi_lib):
    import ccmi
    data = [FILES[0].read_bytes()]
    keep, sp, ln = _args(data)
    plan = _plan(ccmi_lib)
    geom, need = (Geom * 1)(), C.c_size_t(0)
    assert plan(sp, ln, 1, 0, 0, U8, geom, C.byref(need)) == 0, ccmi.last_error()
    for what, rc in (
        ("u8 at 10 bits", plan(sp, ln, 1, 10, 0, U8, geom, C.byref(need))),
        ("unknown sample type", plan(sp, ln, 1, 0, 0, 3, geom, C.byref(need))),
        ("negative sample type", plan(sp, ln, 1, 0, 0, -1, geom, C.byref(need))),
        ("bitdepth 17", plan(sp, ln, 1, 17, 0, U16, geom, C.byref(need))),
        ("chroma 422", plan(sp, ln, 1, 0, 422, U16, geom, C.byref(need))),
        ("n = 0", plan(sp, ln, 0, 0, 0, U8, geom, C.byref(need))),
    ):
        assert rc != 0 and ccmi.last_error(), what
    assert plan(sp, ln, 1, 10, 0, U8, geom, C.byref(need)) == ccmi.ERR_ARG
    assert plan(None, ln, 1, 0, 0, U8, geom, C.byref(need)) != 0 and "null" in ccmi.last_error()
    assert plan(sp, ln, 1, 0, 0, U8, None, C.byref(need)) != 0 and "null" in ccmi.last_error()
    short = C.create_string_buffer(data[0][:60], 60)
    sp1 = (C.c_void_p * 1)(C.cast(short, C.c_void_p))
    ln1 = (C.c_size_t * 1)(60)
    assert plan(sp1, ln1, 1, 0, 0, U8, geom, C.byref(need)) != 0 and ccmi.last_error()


def test_dev_decode_argument_errors_need_no_device(ccmi_lib):
    """ccmi_decode_batch_dev rejects null arguments, n < 1, a short capacity, a null or
    misaligned output pointer and a wrong sample type from the headers alone, before any HIP call."""
    import ccmi
    data = [FILES[0].read_bytes()]
    keep, sp, ln = _args(data)
    dec = ccmi_lib.ccmi_decode_batch_dev
    dec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                    C.c_size_t, C.c_void_p]
    dec.restype = C.c_int
    geom, need = (Geom * 1)(), C.c_size_t(0)
    assert _plan(ccmi_lib)(sp, ln, 1, 0, 0, U16, geom, C.byref(need)) == 0
    out = (C.c_void_p * 1)(0x1000)  # never dereferenced: every call below fails its checks first
    cap = (C.c_size_t * 1)(2 * geom[0].elems)
    short = (C.c_size_t * 1)(2 * geom[0].elems - 1)
    odd = (C.c_void_p * 1)(0x1001)
    null = (C.c_void_p * 1)(None)
    for what, rc in (
        ("null streams", dec(None, ln, 1, out, cap, U16, 0, 0, None, 0, None)),
        ("null outputs", dec(sp, ln, 1, None, cap, U16, 0, 0, None, 0, None)),
        ("null capacities", dec(sp, ln, 1, out, None, U16, 0, 0, None, 0, None)),
        ("n = 0", dec(sp, ln, 0, out, cap, U16, 0, 0, None, 0, None)),
        ("short capacity", dec(sp, ln, 1, out, short, U16, 0, 0, None, 0, None)),
        ("null output pointer", dec(sp, ln, 1, null, cap, U16, 0, 0, None, 0, None)),
        ("misaligned u16 output", dec(sp, ln, 1, odd, cap, U16, 0, 0, None, 0, None)),
        ("unknown sample type", dec(sp, ln, 1, out, cap, 7, 0, 0, None, 0, None)),
        ("u8 at 10 bits", dec(sp, ln, 1, out, cap, U8, 10, 0, None, 0, None)),
    ):
        assert rc == ccmi.ERR_ARG and ccmi.last_error(), what
