"""ccmi_latents_compact_plan / _measure / compact, ccmi_latents_concat and
ccmi_latents_stream_info: the host side.  No compute here (CPU hosts have no HIP device): every
handle is plan-only, built as tests/test_latent_store_abi.py builds them, and every GPU entry
point must refuse before its first HIP call."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
COOL = ROOT / "tests" / "golden" / "cool"
U8, U16, F32 = 0, 1, 2
I8, I16, I32, SEG = 0, 1, 2, 3
MAX_GRIDS = 8
P, I, Z = C.c_void_p, C.c_int, C.c_size_t
NAMES = ["D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool", "E-Johnny-lmbda-0004_1280x720_60p_yuv420_8b.cool",
         "B-BQTerrace-lmbda-0001_1920x1080_50p_yuv420_8b.cool"]


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


@pytest.fixture(scope="module")
def L(ccmi_lib):
    lib = ccmi_lib
    lib.ccmi_latents_plan.argtypes = [P, P, I, I, P, P, P]
    lib.ccmi_latents_decode.argtypes = [P, P, I, I, P, Z, P, Z, P, P]
    lib.ccmi_latents_free.argtypes = [P]
    lib.ccmi_latents_free.restype = None
    lib.ccmi_latents_count.argtypes = [P]
    lib.ccmi_latents_values.argtypes = [P, I, P, Z, P]
    lib.ccmi_latents_render_plan.argtypes = [P, P, I, P, I, I, I, P, P, P]
    lib.ccmi_latents_render.argtypes = [P, P, I, P, P, P, I, I, I, P, Z, P]
    lib.ccmi_latents_compact_plan.argtypes = [P, P, P]
    lib.ccmi_latents_compact_measure.argtypes = [P, P, Z, P, P, P]
    lib.ccmi_latents_compact.argtypes = [P, P, Z, P, Z, P, P]
    lib.ccmi_latents_concat.argtypes = [P, I, P]
    lib.ccmi_latents_stream_info.argtypes = [P, I, P, P]
    for f in (lib.ccmi_latents_plan, lib.ccmi_latents_decode, lib.ccmi_latents_count, lib.ccmi_latents_values,
              lib.ccmi_latents_render_plan, lib.ccmi_latents_render, lib.ccmi_latents_compact_plan,
              lib.ccmi_latents_compact_measure, lib.ccmi_latents_compact, lib.ccmi_latents_concat,
              lib.ccmi_latents_stream_info):
        f.restype = C.c_int
    return lib


def _handle(lib, data, ltype=I16):
    """A plan-only handle over `data` (store = NULL: no GPU call)."""
    import ccmi
    h = C.c_void_p(None)
    keep, sp, ln = _args(data)
    rc = lib.ccmi_latents_decode(sp, ln, len(data), ltype, None, 0, None, 0, None, C.byref(h))
    assert rc == 0 and h.value, ccmi.last_error()
    return h


def _plan(lib, h, index, rects, sample=U16):
    m = len(index)
    geom, info, need = (Geom * m)(), (Info * m)(), C.c_size_t(0)
    idx = (C.c_int * m)(*index)
    arr = None if rects is None else (Rect * m)(*[Rect(*r) for r in rects])
    rc = lib.ccmi_latents_render_plan(h, idx, m, arr, 0, 0, sample, geom, info, C.byref(need))
    return rc, geom, info, need.value


def _fields(s):
    out = []
    for k, _ in s._fields_:
        v = getattr(s, k)
        out.append(list(v) if hasattr(v, "__len__") else v)
    return out


@pytest.fixture(scope="module")
def data():
    return [(COOL / n).read_bytes() for n in NAMES]


def test_compact_plan_bound(L, data):
    """store_bytes_max >= the I32 plan's bytes + 4 bytes per segment of the non-empty grids, the
    same from a handle of any type, and below that plus the alignment allowance."""
    import ccmi
    from ccmi import encode
    keep, sp, ln = _args(data)
    n = len(data)
    tot32, need, each32 = C.c_size_t(0), C.c_size_t(0), (C.c_size_t * n)()
    assert L.ccmi_latents_plan(sp, ln, n, I32, C.byref(tot32), each32, C.byref(need)) == 0, ccmi.last_error()
    segs = coded_grids = 0
    for d in data:
        fr = encode.parse(d)
        for (h, w), nb in zip(fr.grid_sizes, fr.desc.n_bytes_latent[: fr.desc.n_grids]):
            if nb > 0:
                segs += h * ((w + 63) // 64)
                coded_grids += 1
    got = {}
    for t in (I8, I16, I32):
        h = _handle(L, data, t)
        bound, ws = C.c_size_t(0), C.c_size_t(0)
        assert L.ccmi_latents_compact_plan(h, C.byref(bound), C.byref(ws)) == 0, ccmi.last_error()
        L.ccmi_latents_free(h)
        got[t] = (bound.value, ws.value)
        assert bound.value % 256 == 0
        assert bound.value >= tot32.value + 4 * segs
        assert bound.value <= tot32.value + 4 * segs + 16 * coded_grids + 256 * n
        assert ws.value >= 4 * segs and ws.value % 256 == 0  # a word per segment, and the job tables
    assert got[I8] == got[I16] == got[I32]
    print(f"{n} streams: I32 store {tot32.value} bytes, {segs} segments, compact bound {got[I16][0]}, workspace {got[I16][1]}")


def test_argument_errors(L, data):
    import ccmi
    ERR = ccmi.ERR_ARG
    a, b = C.c_size_t(7), C.c_size_t(7)
    out = C.c_void_p(0x1234)
    # NULL source
    assert L.ccmi_latents_compact_plan(None, C.byref(a), C.byref(b)) == ERR and "NULL" in ccmi.last_error()
    assert L.ccmi_latents_compact_measure(None, None, 0, None, C.byref(a), None) == ERR and "NULL" in ccmi.last_error()
    assert L.ccmi_latents_compact(None, 0x1000, 1 << 20, None, 0, None, C.byref(out)) == ERR and "NULL" in ccmi.last_error()
    assert out.value is None  # no handle
    h = _handle(L, data[:1])
    try:
        assert L.ccmi_latents_compact_plan(h, None, C.byref(b)) == ERR
        assert L.ccmi_latents_compact_plan(h, C.byref(a), None) == ERR
        # a plan-only source where the GPU is needed: refused before any HIP call (this host has no GPU)
        assert L.ccmi_latents_compact_measure(h, None, 0, None, C.byref(a), None) == ERR
        assert "plan-only" in ccmi.last_error(), ccmi.last_error()
        out = C.c_void_p(0x1234)
        assert L.ccmi_latents_compact(h, 0x1000, 1 << 20, None, 0, None, C.byref(out)) == ERR
        assert "plan-only" in ccmi.last_error() and out.value is None
        # stream_info
        t, nb = C.c_int(-1), C.c_size_t(0)
        assert L.ccmi_latents_stream_info(h, 0, C.byref(t), C.byref(nb)) == 0 and t.value == I16 and nb.value % 256 == 0
        assert L.ccmi_latents_stream_info(h, 0, None, None) == 0
        assert L.ccmi_latents_stream_info(h, 1, C.byref(t), C.byref(nb)) == ERR and "stream 1" in ccmi.last_error()
        assert L.ccmi_latents_stream_info(h, -1, C.byref(t), C.byref(nb)) == ERR
        assert L.ccmi_latents_stream_info(None, 0, C.byref(t), C.byref(nb)) == ERR and "NULL" in ccmi.last_error()
        # concat
        out = C.c_void_p(0x1234)
        parts = (C.c_void_p * 2)(h, None)
        assert L.ccmi_latents_concat(parts, 0, C.byref(out)) == ERR and "n_parts" in ccmi.last_error()
        assert out.value is None
        assert L.ccmi_latents_concat(parts, -3, C.byref(out)) == ERR
        assert L.ccmi_latents_concat(parts, 2, C.byref(out)) == ERR and "part 1" in ccmi.last_error()
        assert L.ccmi_latents_concat(None, 1, C.byref(out)) == ERR
        assert L.ccmi_latents_concat(parts, 1, None) == ERR
    finally:
        L.ccmi_latents_free(h)


def test_type_3_is_still_not_built_from_streams(L, data):
    import ccmi
    keep, sp, ln = _args(data)
    tot, need = C.c_size_t(0), C.c_size_t(0)
    assert L.ccmi_latents_plan(sp, ln, len(data), SEG, C.byref(tot), None, C.byref(need)) == ccmi.ERR_ARG
    assert "ccmi_latents_compact" in ccmi.last_error(), ccmi.last_error()
    h = C.c_void_p(None)
    assert L.ccmi_latents_decode(sp, ln, len(data), SEG, None, 0, None, 0, None, C.byref(h)) == ccmi.ERR_ARG
    assert "ccmi_latents_compact" in ccmi.last_error() and not h.value
    assert L.ccmi_latents_plan(sp, ln, len(data), 4, C.byref(tot), None, C.byref(need)) == ccmi.ERR_ARG


def test_concat_of_plan_only_handles(L, data):
    """Count, per-stream info, and render_plan geometry / info / workspace for an index across
    the parts equal to those of the parts' own plans (and to one handle over all the streams)."""
    import ccmi
    parts_data = [data[:1], data[1:], data[:2]]  # 1 + 2 + 2 streams
    types = [I16, I8, I32]
    hs = [_handle(L, d, t) for d, t in zip(parts_data, types)]
    arr = (C.c_void_p * 3)(*hs)
    cat = C.c_void_p(None)
    assert L.ccmi_latents_concat(arr, 3, C.byref(cat)) == 0 and cat.value, ccmi.last_error()
    flat = [(p, i) for p, d in enumerate(parts_data) for i in range(len(d))]
    assert L.ccmi_latents_count(cat) == 5
    info_parts = []
    for p, i in flat:
        t, nb = C.c_int(-1), C.c_size_t(0)
        assert L.ccmi_latents_stream_info(hs[p], i, C.byref(t), C.byref(nb)) == 0
        info_parts.append((t.value, nb.value))
        assert t.value == types[p]
    index = [4, 0, 2, 2, 1, 3]
    rects = [(512, 232, 256, 256), (0, 0, 64, 64), (1600, 800, 256, 256), (2, 4, 65, 33), (0, 0, 1280, 720), (80, 48, 256, 128)]
    per_part = []
    for j, r in zip(index, rects):
        p, i = flat[j]
        rc, g, info, need = _plan(L, hs[p], [i], [r])
        assert rc == 0, ccmi.last_error()
        per_part.append((_fields(g[0]), _fields(info[0]), need))
    # the parts may be freed: the new handle stands alone
    for h in hs:
        L.ccmi_latents_free(h)
    try:
        for k, (p, i) in enumerate(flat):
            t, nb = C.c_int(-1), C.c_size_t(0)
            assert L.ccmi_latents_stream_info(cat, k, C.byref(t), C.byref(nb)) == 0
            assert (t.value, nb.value) == info_parts[k]
        rc, g, info, need = _plan(L, cat, index, rects)
        assert rc == 0, ccmi.last_error()
        for j in range(len(index)):
            assert _fields(g[j]) == per_part[j][0] and _fields(info[j]) == per_part[j][1], j
        # each frame alone: the part's own workspace figure; and the storage type does not enter a render plan
        for j in range(len(index)):
            rc, g1, i1, need1 = _plan(L, cat, [index[j]], [rects[j]])
            assert rc == 0 and need1 == per_part[j][2], j
        one = _handle(L, [parts_data[flat[j][0]][flat[j][1]] for j in range(5)], I16)
        rc, g2, i2, need2 = _plan(L, one, index, rects)
        L.ccmi_latents_free(one)
        assert rc == 0 and need2 == need
        # plan-only stays plan-only: no render, no values, no measure; a concat of a concat works
        out, cap, idx = (C.c_void_p * 1)(0x1000), (C.c_size_t * 1)(1 << 20), (C.c_int * 1)(0)
        assert L.ccmi_latents_render(cat, idx, 1, None, out, cap, U8, 0, 0, None, 0, None) == ccmi.ERR_ARG
        assert "plan-only" in ccmi.last_error()
        assert L.ccmi_latents_values(cat, 0, 0x1000, 1 << 30, None) == ccmi.ERR_ARG and "plan-only" in ccmi.last_error()
        a = C.c_size_t(0)
        assert L.ccmi_latents_compact_measure(cat, None, 0, None, C.byref(a), None) == ccmi.ERR_ARG
        bound, ws = C.c_size_t(0), C.c_size_t(0)
        assert L.ccmi_latents_compact_plan(cat, C.byref(bound), C.byref(ws)) == 0 and bound.value > 0
        two = (C.c_void_p * 2)(cat, cat)
        cc = C.c_void_p(None)
        assert L.ccmi_latents_concat(two, 2, C.byref(cc)) == 0 and L.ccmi_latents_count(cc) == 10
        rc, g3, i3, need3 = _plan(L, cc, [9, 5], [rects[0], rects[1]])
        assert rc == 0 and _fields(g3[0]) == per_part[0][0] and _fields(g3[1]) == per_part[1][0]
        L.ccmi_latents_free(cc)
        rc, _, _, _ = _plan(L, cat, [5], None)
        assert rc == ccmi.ERR_ARG and "frame 0" in ccmi.last_error()
    finally:
        L.ccmi_latents_free(cat)


def test_exported_symbols(L):
    import ccmi
    for name in ("ccmi_latents_compact_plan", "ccmi_latents_compact_measure", "ccmi_latents_compact",
                 "ccmi_latents_concat", "ccmi_latents_stream_info"):
        assert name in ccmi.EXPORTED and hasattr(L, name)
