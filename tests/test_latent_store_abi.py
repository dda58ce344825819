"""ccmi_latents_*: the host side of the latent store (decode once, render often).  No compute
here (CPU hosts have no HIP device): every handle is plan-only (ccmi_latents_decode with
store = NULL parses the headers, decodes the networks on the host and makes no GPU call).  The
store's layout against the documented bounds, the render planning against the region decode's
planning for the same streams and arguments, the index list, and the argument errors."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
COOL = ROOT / "tests" / "golden" / "cool"
FILES = sorted(COOL.rglob("*.cool"))
U8, U16, F32 = 0, 1, 2
I8, I16, I32 = 0, 1, 2
MAX_GRIDS = 8
P, I, Z = C.c_void_p, C.c_int, C.c_size_t


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
    lib.ccmi_latents_render_plan.argtypes = [P, P, I, P, I, I, I, P, P, P]
    lib.ccmi_latents_render.argtypes = [P, P, I, P, P, P, I, I, I, P, Z, P]
    lib.ccmi_decode_batch_dev_plan.argtypes = [P, P, I, I, I, I, P, P]
    lib.ccmi_decode_batch_dev_roi_plan.argtypes = [P, P, I, P, I, I, I, P, P, P]
    for f in (lib.ccmi_latents_plan, lib.ccmi_latents_decode, lib.ccmi_latents_count, lib.ccmi_latents_render_plan,
              lib.ccmi_latents_render, lib.ccmi_decode_batch_dev_plan, lib.ccmi_decode_batch_dev_roi_plan):
        f.restype = C.c_int
    return lib


class Handle:
    """A plan-only handle over `data` (store = NULL: no GPU call)."""

    def __init__(self, lib, data, ltype=I16):
        import ccmi
        self.lib, self.h = lib, C.c_void_p(None)
        keep, sp, ln = _args(data)
        rc = lib.ccmi_latents_decode(sp, ln, len(data), ltype, None, 0, None, 0, None, C.byref(self.h))
        assert rc == 0 and self.h.value, ccmi.last_error()
        # the handle does not refer to the streams after the call: overwrite and drop them
        for b in keep:
            C.memset(b, 0xA5, len(b))
        del keep, sp, ln

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.ccmi_latents_free(self.h)

    def plan(self, index, rects, bitdepth=0, chroma=0, sample=U16, m=None):
        """(rc, geom, info, workspace bytes) of one ccmi_latents_render_plan call."""
        if m is None:
            m = len(index) if index is not None else self.lib.ccmi_latents_count(self.h)
        k = max(m, 1)
        geom, info, need = (Geom * k)(), (Info * k)(), C.c_size_t(0)
        idx = None if index is None else (C.c_int * k)(*index)
        arr = None if rects is None else (Rect * k)(*[Rect(*r) for r in rects])
        rc = self.lib.ccmi_latents_render_plan(self.h, idx, m, arr, bitdepth, chroma, sample, geom, info, C.byref(need))
        return rc, geom, info, need.value


def _roi_plan(lib, data, rects, bitdepth=0, chroma=0, sample=U16):
    n = len(data)
    keep, sp, ln = _args(data)
    geom, info, need = (Geom * n)(), (Info * n)(), C.c_size_t(0)
    arr = None if rects is None else (Rect * n)(*[Rect(*r) for r in rects])
    rc = lib.ccmi_decode_batch_dev_roi_plan(sp, ln, n, arr, bitdepth, chroma, sample, geom, info, C.byref(need))
    return rc, geom, info, need.value


def _fields(s):
    out = []
    for k, _ in s._fields_:
        v = getattr(s, k)
        out.append(list(v) if hasattr(v, "__len__") else v)
    return out


def test_store_plan_sizes_and_padding_bound(L):
    """Per stream: 4 (ups + syn) + N' sizeof(T) <= store_bytes_each <= 4 (ups + syn + blend) +
    N sizeof(T) + 256 (n_grids + 4), N' = the latents of the non-empty grids; 256-byte
    multiples whose sum is store_bytes; I8 < I16 < I32."""
    import ccmi
    from ccmi import encode
    assert len(FILES) > 30
    data = [f.read_bytes() for f in FILES]
    n = len(data)
    keep, sp, ln = _args(data)
    each = {}
    total = {}
    ws = {}
    for t, eb in ((I8, 1), (I16, 2), (I32, 4)):
        tot, need, arr = C.c_size_t(0), C.c_size_t(0), (C.c_size_t * n)()
        assert L.ccmi_latents_plan(sp, ln, n, t, C.byref(tot), arr, C.byref(need)) == 0, ccmi.last_error()
        each[t], total[t], ws[t] = list(arr), tot.value, need.value
        assert tot.value == sum(arr) and all(a % 256 == 0 and a > 0 for a in arr)
        tot2 = C.c_size_t(0)
        assert L.ccmi_latents_plan(sp, ln, n, t, C.byref(tot2), None, C.byref(need)) == 0 and tot2.value == tot.value
        empties = 0
        for f, d, got in zip(FILES, data, arr):
            fr = encode.parse(d)
            desc = fr.desc
            ups = desc.n_ups * desc.ups_k + desc.n_pre * desc.pre_k
            blend = desc.n_branches if desc.n_branches > 1 else 0
            syn = fr.nn["syn_w"].size + fr.nn["syn_b"].size - blend
            sizes = [h * w for h, w in fr.grid_sizes]
            coded = [s for s, nb in zip(sizes, desc.n_bytes_latent[: desc.n_grids]) if nb > 0]
            empties += len(sizes) - len(coded)
            assert got >= 4 * (ups + syn) + sum(coded) * eb, f.name
            assert got <= 4 * (ups + syn + blend) + sum(sizes) * eb + 256 * (desc.n_grids + 4), f.name
            # an empty grid takes no store bytes at all: the padding allowance of the coded grids alone holds
            assert got <= 4 * (ups + syn + blend) + sum(coded) * eb + 256 * (len(coded) + 4), f.name
        assert empties > 0, "no committed stream with an empty latent grid left"
    assert total[I8] < total[I16] < total[I32]
    assert all(a <= b <= c for a, b, c in zip(each[I8], each[I16], each[I32]))
    assert ws[I8] == ws[I16] == ws[I32]  # the build workspace holds int32 planes whatever the store's type
    tot, need = C.c_size_t(0), C.c_size_t(0)
    assert L.ccmi_latents_plan(sp, ln, n, 3, C.byref(tot), None, C.byref(need)) == ccmi.ERR_ARG
    assert L.ccmi_latents_plan(sp, ln, 0, I16, C.byref(tot), None, C.byref(need)) == ccmi.ERR_ARG


def test_whole_frame_render_plan_is_the_whole_frame_decode_plan(L):
    import ccmi
    for f in FILES:
        data = [f.read_bytes()]
        keep, sp, ln = _args(data)
        g0, need0 = (Geom * 1)(), C.c_size_t(0)
        assert L.ccmi_decode_batch_dev_plan(sp, ln, 1, 0, 0, U16, g0, C.byref(need0)) == 0, ccmi.last_error()
        with Handle(L, data) as h:
            assert L.ccmi_latents_count(h.h) == 1
            for rects in (None, [(0, 0, g0[0].width, g0[0].height)]):
                rc, g, info, need = h.plan(None, rects)
                assert rc == 0, ccmi.last_error()
                assert _fields(g[0]) == _fields(g0[0]), f.name
                assert 0 < need <= need0.value, f.name  # no coded bytes, networks, descriptors or status words


RECTS = [(3, 5, 65, 33), (2, 4, 65, 33), (0, 0, 1, 1), (0, 0, 64, 64), (416 - 64, 240 - 64, 64, 64), (0, 0, 416, 1),
         (0, 0, 416, 8), (80, 48, 256, 128)]


@pytest.mark.parametrize("bitdepth,chroma,sample", [(0, 0, U16), (8, 444, U8), (10, 420, U16), (10, 444, F32)])
def test_region_render_plan_is_the_region_decode_plan(L, bitdepth, chroma, sample):
    """geom and info of ccmi_decode_batch_dev_roi_plan, rect by rect, over the class-D streams
    (both synthesis depths, one with an empty grid) and for 720p / 1080p regions."""
    import ccmi
    d_files = [f for f in FILES if f.name.startswith("D-")]
    data = [f.read_bytes() for f in d_files[:: max(1, len(d_files) // 8)]][:8]
    rects = [r if chroma == 444 else (r[0] & ~1, r[1] & ~1, r[2], r[3]) for r in RECTS[: len(data)]]
    rc0, g0, i0, need0 = _roi_plan(L, data, rects, bitdepth, chroma, sample)
    assert rc0 == 0, ccmi.last_error()
    with Handle(L, data) as h:
        rc, g, info, need = h.plan(None, rects, bitdepth, chroma, sample)
        assert rc == 0, ccmi.last_error()
        for j in range(len(data)):
            assert _fields(g[j]) == _fields(g0[j]), j
            assert _fields(info[j]) == _fields(i0[j]) and info[j].windowed == 1, j
        assert need <= need0
    for name, rect in (("E-Johnny-lmbda-0004_1280x720_60p_yuv420_8b.cool", (512, 232, 256, 256)),
                       ("B-BQTerrace-lmbda-0001_1920x1080_50p_yuv420_8b.cool", (1664, 824, 256, 256))):
        data = [(COOL / name).read_bytes()]
        rc0, g0, i0, need0 = _roi_plan(L, data, [rect], bitdepth, chroma, sample)
        with Handle(L, data) as h:
            rc, g, info, need = h.plan([0], [rect], bitdepth, chroma, sample)
            assert rc == rc0 == 0, ccmi.last_error()
            assert _fields(g[0]) == _fields(g0[0]) and _fields(info[0]) == _fields(i0[0])


def test_index_selects_the_stream_of_each_frame(L):
    import ccmi
    names = ["D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool", "E-Johnny-lmbda-0004_1280x720_60p_yuv420_8b.cool",
             "B-BQTerrace-lmbda-0001_1920x1080_50p_yuv420_8b.cool"]
    sizes = [(416, 240), (1280, 720), (1920, 1080)]
    data = [(COOL / n).read_bytes() for n in names]
    with Handle(L, data) as h:
        assert L.ccmi_latents_count(h.h) == 3
        index = [2, 0, 2, 1]
        rc, g, info, need = h.plan(index, None)
        assert rc == 0, ccmi.last_error()
        assert [(g[j].width, g[j].height) for j in range(4)] == [sizes[i] for i in index]
        # a region per frame: the info of a region decode of the streams in that order
        rects = [(1600, 800, 256, 256), (0, 0, 64, 64), (0, 0, 256, 256), (512, 232, 256, 256)]
        rc, g, info, need = h.plan(index, rects)
        rc0, g0, i0, need0 = _roi_plan(L, [data[i] for i in index], rects)
        assert rc == rc0 == 0, ccmi.last_error()
        for j in range(4):
            assert _fields(g[j]) == _fields(g0[j]) and _fields(info[j]) == _fields(i0[j]), j
        # without an index m must be the handle's count
        assert h.plan(None, None, m=2)[0] == ccmi.ERR_ARG
        assert h.plan(None, None, m=3)[0] == 0


def test_argument_errors_name_the_frame(L):
    import ccmi
    name = "D-BQSquare-lmbda-0001_416x240_60p_yuv420_8b.cool"
    data = [(COOL / name).read_bytes()] * 3
    ok = (0, 0, 16, 16)
    with Handle(L, data) as h:
        for what, index, rects, kw in (
            ("index -1", [0, 0, -1], None, {}),
            ("index n", [0, 0, 3], None, {}),
            ("a region outside the frame", [0, 1, 2], [ok, ok, (416 - 15, 0, 16, 16)], {"chroma": 444}),
            ("an odd origin at 420", [0, 1, 2], [ok, ok, (3, 4, 16, 16)], {"chroma": 420}),
            ("U8 with a 10-bit output", [2, 1, 0], None, {"bitdepth": 10, "sample": U8}),
        ):
            rc, g, info, need = h.plan(index, rects, **kw)
            assert rc == ccmi.ERR_ARG, what
            want = "frame 0" if what.startswith("U8") else "frame 2"
            assert want in ccmi.last_error(), (what, ccmi.last_error())
        rc, g, info, need = h.plan([], None, m=0)
        assert rc == ccmi.ERR_ARG and "m < 1" in ccmi.last_error(), ccmi.last_error()
        # a plan-only handle cannot render; the check comes before any HIP call (this host has no GPU)
        out = (C.c_void_p * 1)(0x1000)  # never dereferenced
        cap = (C.c_size_t * 1)(1 << 20)
        idx = (C.c_int * 1)(0)
        rc = L.ccmi_latents_render(h.h, idx, 1, None, out, cap, U8, 0, 0, None, 0, None)
        assert rc == ccmi.ERR_ARG and "plan-only" in ccmi.last_error() and "frame" in ccmi.last_error()
    # a NULL handle
    geom, need = (Geom * 1)(), C.c_size_t(0)
    idx = (C.c_int * 1)(0)
    assert L.ccmi_latents_render_plan(None, idx, 1, None, 0, 0, U16, geom, None, C.byref(need)) == ccmi.ERR_ARG
    assert "frame" in ccmi.last_error()
    out, cap = (C.c_void_p * 1)(0x1000), (C.c_size_t * 1)(1 << 20)
    assert L.ccmi_latents_render(None, idx, 1, None, out, cap, U8, 0, 0, None, 0, None) == ccmi.ERR_ARG
    assert L.ccmi_latents_count(None) == 0
    L.ccmi_latents_free(None)


def test_render_workspace_is_not_larger_than_the_region_decodes(L):
    e_files = [f for f in FILES if f.name.startswith("E-")]
    assert len(e_files) >= 10
    data = [f.read_bytes() for f in e_files]
    rects = [(2 * ((37 * k) % 512), 2 * ((53 * k) % 232), 256, 256) for k in range(len(data))]
    rc0, g0, i0, need0 = _roi_plan(L, data, rects)
    with Handle(L, data) as h:
        rc, g, info, need = h.plan(None, rects)
    assert rc == rc0 == 0
    assert 0 < need <= need0, f"render workspace {need} bytes, region decode {need0} bytes"
    print(f"{len(data)} class-E streams, 256x256 regions: render workspace {need} bytes, region decode {need0} bytes")
