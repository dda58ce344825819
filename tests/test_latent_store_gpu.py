"""Latent store (ccmi_latents_* / decode.LatentStore): decode once, render regions often.

The reference is always code that existed before the store: decode.decode_latents for the
values, and for the samples the bytes of decode.decode_batch (pinned elsewhere to the reference
decoder's md5s and the C oracle), cropped in numpy as tests/test_decode_roi_gpu.py does --
never decode_batch_tensors(roi=...) and never the store itself.

The generated streams are the region tests': 21 x 37, 34 x 66 and 21 x 37 with a generic
synthesis (per-frame tail, cropping output kernel).  Their coarse grids are 1 to 5 samples
wide, so most grids are smaller than one 16-byte group of the pack kernel.  Render workspaces
are filled with 0xA5 or 0x5A: a plane sample the unpack did not write but the tail reads shows
as a mismatch in one of the two."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import synth_streams as S

GOLDEN = Path(__file__).resolve().parent / "golden"
FILES = sorted((GOLDEN / "cool").glob("*.cool"))
SMALL = ((21, 37), (34, 66), (21, 37))  # the last one with the generic synthesis
I8, I16, I32 = 0, 1, 2
NARROW = 32

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _planes(b, h, w, bitdepth, chroma):
    """decode_batch's .yuv bytes -> [Y, U, V] numpy planes."""
    a = np.frombuffer(b, dtype="u1" if bitdepth <= 8 else "<u2")
    if chroma == 444:
        assert a.size == 3 * h * w
        return list(a.reshape(3, h, w))
    ch, cw = h // 2, w // 2
    assert a.size == h * w + 2 * ch * cw
    return [a[: h * w].reshape(h, w), a[h * w: h * w + ch * cw].reshape(ch, cw), a[h * w + ch * cw:].reshape(ch, cw)]


def _crop(planes, rect, chroma):
    x, y, w, h = rect
    if chroma == 444:
        return [p[y: y + h, x: x + w] for p in planes]
    assert x % 2 == 0 and y % 2 == 0
    return [planes[0][y: y + h, x: x + w]] + [p[y // 2: y // 2 + h // 2, x // 2: x // 2 + w // 2] for p in planes[1:]]


def _item_planes(item):
    if isinstance(item, dict):
        return [_np(item[k]) for k in "yuv"]
    return list(_np(item))


def _same(item, planes, rect, chroma, what):
    want = _crop(planes, rect, chroma)
    got = _item_planes(item)
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape, (what, rect, k, g.shape, r.shape)
        assert np.array_equal(g, r), (what, rect, "plane %d" % k, int((g != r).sum()), "samples differ")


def _generate(h, w, seed, generic=False, plants=(), zero_grid=None):
    """The region tests' recipe; plants: ((grid, flat index or -1 for the last sample, value), ...)."""
    import torch
    from ccmi import encode
    fr = encode.parse(S.BASE.read_bytes())
    d = fr.desc
    d.h, d.w = h, w
    if generic:
        c_in, p, parts = d.n_grids, 0, []
        assert d.n_syn_layers >= 3 and d.syn_ks[2] == 3 and d.n_branches == 1
        for l in range(d.n_syn_layers):
            n = d.syn_out[l] * c_in * d.syn_ks[l] ** 2
            wl = fr.nn["syn_w"][p: p + n]
            if l == 2:
                wl = wl.reshape(d.syn_out[l], c_in, 3, 3)[:, :, 1, 1].reshape(-1)
            parts.append(wl)
            p, c_in = p + n, d.syn_out[l]
        fr.nn["syn_w"] = np.concatenate(parts)
        d.syn_ks[2] = 1
    g = torch.Generator().manual_seed(seed)
    lat = [torch.round(2.0 * torch.randn(hh * ww, generator=g)).to(torch.int32) for hh, ww in fr.grid_sizes]
    if zero_grid is not None:
        lat[zero_grid][:] = 0
    for grid, at, v in plants:
        lat[grid][at] = v
    d.ac_max_val_latent = min(65535, max(int(a.abs().max()) for a in lat) + 2)
    return encode.encode_frame(fr, torch.cat(lat).cuda(), search_counts=True)


@pytest.fixture(scope="module")
def small(gpu, ccmi_lib):
    return [_generate(21, 37, 7), _generate(34, 66, 9), _generate(21, 37, 11, generic=True)]


@pytest.fixture(scope="module")
def small_ref(small, gpu, ccmi_lib):
    """{(bitdepth, chroma): [planes of every generated stream]} from decode_batch."""
    from ccmi import decode
    ref = {}
    for bitdepth, chroma in ((8, 420), (8, 444), (10, 420), (10, 444)):
        outs = decode.decode_batch(small, output_bitdepth=bitdepth, output_chroma_format=chroma, as_yuv=True)
        ref[(bitdepth, chroma)] = [_planes(r, h, w, bitdepth, chroma) for r, (h, w) in zip(outs, SMALL)]
    return ref


@pytest.fixture(scope="module")
def class_d(gpu, ccmi_lib):
    """Two committed class-D 416 x 240 streams (the second one has an empty latent grid) and
    their planes at their own format."""
    from ccmi import decode, encode
    d_files = [f for f in FILES if f.name.startswith("D-")]
    empty = [f for f in d_files if 0 in list(encode.parse(f.read_bytes()).desc.n_bytes_latent[:7])]
    assert empty, "no committed class-D stream with an empty latent grid left"
    files = [d_files[0] if d_files[0] != empty[0] else d_files[1], empty[0]]
    data = [f.read_bytes() for f in files]
    outs = decode.decode_batch(data, as_yuv=True)
    return data, [_planes(o, 240, 416, 8, 420) for o in outs]


@pytest.fixture(scope="module")
def small_store(small, gpu, ccmi_lib):
    from ccmi import decode
    st = decode.LatentStore(small)
    yield st
    st.close()


def _filled_ws(store, fill, **kw):
    import torch
    _, need = store.render_geometry(**kw)
    return torch.full((max(need, 256),), fill, dtype=torch.uint8, device="cuda")


def _c_build(streams, ltype):
    """ccmi_latents_decode itself: the store pre-filled with 0xA5 with 256 guard bytes after
    store_bytes, the build workspace filled with 0xA5 too.  -> (rc, handle, store tensor,
    store_bytes, workspace tensor)."""
    import torch
    from ccmi import decode
    L = decode._bind_latents()
    n = len(streams)
    keep, sp, ln = decode._marshal(streams)
    nstore, nws = C.c_size_t(0), C.c_size_t(0)
    each = (C.c_size_t * n)()
    decode.check(L.ccmi_latents_plan(sp, ln, n, ltype, C.byref(nstore), each, C.byref(nws)))
    assert sum(each) == nstore.value
    store = torch.full((nstore.value + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((max(nws.value, 256),), 0xA5, dtype=torch.uint8, device="cuda")
    h = C.c_void_p(None)
    rc = L.ccmi_latents_decode(sp, ln, n, ltype, store.data_ptr(), nstore.value, ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream().cuda_stream, C.byref(h))
    torch.cuda.synchronize()
    return rc, h, store, nstore.value, ws


def _c_values(h, i, sizes):
    import torch
    from ccmi import decode
    n = sum(a * b for a, b in sizes)
    flat = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    decode.check(decode._bind_latents().ccmi_latents_values(h, i, flat.data_ptr(), n,
                                                            torch.cuda.current_stream().cuda_stream))
    host = _np(flat)
    assert (host[n:] == 0x5A5A5A5A).all()
    out, p = [], 0
    for a, b in sizes:
        out.append(host[p: p + a * b])
        p += a * b
    return out


@pytest.mark.parametrize("ltype", [I8, I16, I32])
def test_values_are_decode_latents_and_the_guard_bytes_stay(ltype, small, class_d, gpu, ccmi_lib):
    """ccmi_latents_values and LatentStore.latents against decode_latents: the generated streams
    at every element type, the class-D streams (one with an empty grid) at int16 and int32."""
    import torch
    from ccmi import decode, encode
    streams = list(small) + (list(class_d[0]) if ltype != I8 else [])
    want = [decode.decode_latents(s) for s in streams]
    rc, h, store, nbytes, ws = _c_build(streams, ltype)
    try:
        assert rc == 0 and h.value, decode.lib().ccmi_last_error()
        assert (_np(store[nbytes:]) == 0xA5).all(), "the 256 guard bytes after store_bytes were written"
        assert decode.last_arm_flags() == [0] * len(streams) or all(not f & NARROW for f in decode.last_arm_flags())
        for i, s in enumerate(streams):
            sizes = encode.parse(s).grid_sizes
            got = _c_values(h, i, sizes)
            for l, (g, w) in enumerate(zip(got, want[i])):
                assert np.array_equal(g, w.reshape(-1)), (i, l, int((g != w.reshape(-1)).sum()))
    finally:
        decode._bind_latents().ccmi_latents_free(h)
    st = decode.LatentStore(streams, dtype=(torch.int8, torch.int16, torch.int32)[ltype])
    assert len(st) == len(streams) and st.dtype == (torch.int8, torch.int16, torch.int32)[ltype] and st.nbytes == nbytes
    assert [(g["width"], g["height"]) for g in st.geometry[:3]] == [(w, h) for h, w in SMALL]
    for i, s in enumerate(streams):
        got = st.latents(i)
        assert [tuple(t.shape) for t in got] == [tuple(x) for x in encode.parse(s).grid_sizes]
        for l, (g, w) in enumerate(zip(got, want[i])):
            assert g.dtype == torch.int32 and np.array_equal(_np(g).reshape(-1), w.reshape(-1)), (i, l)
    st.close()


BOUNDARY = [(127, I8, True), (-128, I8, True), (128, I8, False), (-129, I8, False), (32767, I16, True),
            (-32768, I16, True), (32768, I16, False), (32768, I32, True)]


@pytest.fixture(scope="module")
def planted(gpu, ccmi_lib):
    """21 x 37 streams with one planted latent: at the last sample of grid 0, or in the coarsest
    grid; every other latent is N(0, 2) (|q| far below 127)."""
    made = {}

    def get(value, where):
        if (value, where) not in made:
            plant = (0, -1, value) if where == "grid0-last" else (6, 0, value)
            made[(value, where)] = _generate(21, 37, 21, plants=(plant,))
        return made[(value, where)]
    return get


@pytest.mark.parametrize("where", ["grid0-last", "coarsest"])
@pytest.mark.parametrize("value,ltype,fits", BOUNDARY)
def test_type_boundaries(value, ltype, fits, where, small, planted, gpu, ccmi_lib):
    """A latent that does not fit the element type is never saturated or wrapped: the build
    fails with CCMI_ERR_UNSUPPORTED, NARROW is set for that stream only, no handle exists."""
    import ccmi
    from ccmi import decode, encode
    s = planted(value, where)
    lat = decode.decode_latents(s)
    assert (lat[0][-1] if where == "grid0-last" else lat[6][0]) == value
    rc, h, store, nbytes, ws = _c_build([small[0], s, small[0]], ltype)
    flags = decode.last_arm_flags()
    try:
        if fits:
            assert rc == 0 and h.value, decode.lib().ccmi_last_error()
            assert not any(f & NARROW for f in flags)
            got = _c_values(h, 1, encode.parse(s).grid_sizes)
            for l in range(7):
                assert np.array_equal(got[l], lat[l].reshape(-1)), l
        else:
            msg = ccmi.last_error()
            assert rc == ccmi.ERR_UNSUPPORTED and not h.value, (rc, msg)
            assert [bool(f & NARROW) for f in flags] == [False, True, False], flags
            assert "stream 1" in msg and ("grid 0" if where == "grid0-last" else "grid 6") in msg, msg
            assert ("int8" if ltype == I8 else "int16") in msg, msg
    finally:
        decode._bind_latents().ccmi_latents_free(h)
    assert (_np(store[nbytes:]) == 0xA5).all()


def test_default_dtype_widens_to_int32(small, planted, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    s = planted(32768, "grid0-last")
    streams = [small[0], s, small[1]]
    with pytest.raises(decode.CcmiError) as e:
        decode.LatentStore(streams, dtype=torch.int16)
    assert e.value.code == 3
    st = decode.LatentStore(streams)
    assert st.dtype == torch.int32
    assert decode.LatentStore(small).dtype == torch.int16
    outs = st.render(output_chroma_format=444)
    ref = decode.decode_batch(streams, output_chroma_format=444, as_yuv=True)
    for o, r, (h, w) in zip(outs, ref, (SMALL[0], SMALL[0], SMALL[1])):
        _same(o, _planes(r, h, w, 8, 444), (0, 0, w, h), 444, "widened store")
    st.close()


@pytest.mark.parametrize("bitdepth,chroma", [(8, 420), (8, 444), (10, 420), (10, 444)])
def test_whole_frame_render_is_decode_batch(bitdepth, chroma, small_store, small_ref, gpu, ccmi_lib):
    import torch
    dtypes = [None, torch.uint16, torch.float32] + ([torch.uint8] if bitdepth == 8 else [])
    maxv = np.float32((1 << bitdepth) - 1)
    for dt in dtypes:
        kw = dict(output_bitdepth=bitdepth, output_chroma_format=chroma, dtype=dt)
        outs = small_store.render(workspace=_filled_ws(small_store, 0xA5, **kw), **kw)
        for i, (o, (h, w)) in enumerate(zip(outs, SMALL)):
            want = _crop(small_ref[(bitdepth, chroma)][i], (0, 0, w, h), chroma)
            got = _item_planes(o)
            for g, r in zip(got, want):
                if dt == torch.float32:
                    assert g.tobytes() == (r.astype(np.float32) / maxv).tobytes(), (i, dt)
                else:
                    assert g.dtype == (np.uint16 if dt == torch.uint16 or bitdepth > 8 else np.uint8)
                    assert np.array_equal(g, r), (i, dt)
    if bitdepth == 10:
        from ccmi import decode
        with pytest.raises(decode.CcmiError):
            small_store.render(output_bitdepth=10, dtype=torch.uint8)


def test_class_d_whole_frames_and_the_empty_grid(class_d, gpu, ccmi_lib):
    """The class-D streams at their own format.  The second has an empty latent grid (no store
    bytes): its render and its values are right after a render of the other, non-zero stream
    has used the same workspace."""
    import torch
    from ccmi import decode
    data, planes = class_d
    for dt in (torch.int16, torch.int32):
        st = decode.LatentStore(data, dtype=dt)
        ws = _filled_ws(st, 0xA5)
        a, = st.render(index=[0], workspace=ws)
        _same(a, planes[0], (0, 0, 416, 240), 420, "class D, non-empty")
        b, = st.render(index=[1], workspace=ws)  # the planes now hold stream 0's latents
        _same(b, planes[1], (0, 0, 416, 240), 420, "class D, empty grid")
        rect = (64, 32, 200, 100)
        c, = st.render(index=[0], roi=rect, workspace=ws)
        d, = st.render(index=[1], roi=rect, workspace=ws)
        _same(c, planes[0], rect, 420, "class D region")
        _same(d, planes[1], rect, 420, "class D region, empty grid")
        want = decode.decode_latents(data[1])
        got = st.latents(1)
        assert any(not w.any() for w in want)
        for g, w in zip(got, want):
            assert np.array_equal(_np(g).reshape(-1), w.reshape(-1))
        both = st.render()
        for o, p in zip(both, planes):
            _same(o, p, (0, 0, 416, 240), 420, "class D, both")
        st.close()


def _small_rects(h, w, chroma, seed):
    rects = [(0, 0, w, h)]
    rects += [(0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, h // 2, 1, 1)]
    rects += [(0, 0, w, 1), (0, h - 1, w, 1), (0, 0, 1, h), (w - 1, 0, 1, h)]
    rng = np.random.default_rng(seed)
    for _ in range(24):
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        rects.append((int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))
    if chroma == 420:  # origins rounded down to even, sizes of at least 2 x 2
        out = []
        for x, y, rw, rh in rects:
            x, y = min(x & ~1, (w - 2) & ~1), min(y & ~1, (h - 2) & ~1)
            out.append((x, y, min(max(rw, 2), w - x), min(max(rh, 2), h - y)))
        rects = out
    assert len(rects) == 34
    return rects


@pytest.mark.parametrize("chroma", [444, 420])
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_every_rect_is_the_crop_with_both_workspace_fills(idx, chroma, small_store, small_ref, gpu, ccmi_lib):
    """Corners, strips, the whole frame and 24 seeded rects of each generated frame, rendered
    twice from one store: the workspace pre-filled with 0xA5, then with 0x5A."""
    h, w = SMALL[idx]
    planes = small_ref[(8, chroma)][idx]
    rects = _small_rects(h, w, chroma, 100 + idx)
    index = [idx] * len(rects)
    plan = small_store.roi_plan(index, rects, 8, chroma)
    assert all(p["windowed"] == (idx != 2) for p in plan)  # the generic synthesis takes the crop path
    kw = dict(index=index, roi=rects, output_bitdepth=8, output_chroma_format=chroma)
    for fill in (0xA5, 0x5A):
        outs = small_store.render(workspace=_filled_ws(small_store, fill, **kw), **kw)
        for r, o in zip(rects, outs):
            _same(o, planes, r, chroma, "fill %#x" % fill)
    for r in (rects[4], rects[7], rects[20]):
        kw1 = dict(index=[idx], roi=[r], output_bitdepth=8, output_chroma_format=chroma)
        o, = small_store.render(workspace=_filled_ws(small_store, 0x5A, **kw1), **kw1)
        _same(o, planes, r, chroma, "alone")


def test_index_repeats_and_mixed_sizes(small_store, small_ref, gpu, ccmi_lib):
    index = [2, 0, 2, 1, 2, 0, 0]
    rects = [(3, 5, 9, 7), (0, 0, 37, 21), (10, 2, 20, 19), (17, 9, 40, 22), None, (36, 20, 1, 1), (1, 1, 30, 12)]
    for chroma in (444, 420):
        rr = [r if r is None or chroma == 444 else (r[0] & ~1, r[1] & ~1, max(r[2], 2), max(r[3], 2)) for r in rects]
        rr = [r if r is None else (r[0], r[1], min(r[2], SMALL[i][1] - r[0]), min(r[3], SMALL[i][0] - r[1]))
              for r, i in zip(rr, index)]
        kw = dict(index=index, roi=rr, output_bitdepth=8, output_chroma_format=chroma)
        geom, _ = small_store.render_geometry(**kw)
        outs = small_store.render(workspace=_filled_ws(small_store, 0xA5, **kw), **kw)
        assert len(outs) == len(index) > len(small_store)
        for j, (i, r, o) in enumerate(zip(index, rr, outs)):
            full = (0, 0, SMALL[i][1], SMALL[i][0])
            assert (geom[j]["width"], geom[j]["height"]) == (r or full)[2:]
            _same(o, small_ref[(8, chroma)][i], r or full, chroma, "frame %d" % j)
    # equal-size crops of frames of different sizes, stacked
    rects = [(2 * j, 2 * (j % 3), 12, 10) for j in range(len(index))]
    o444 = small_store.render(index=index, roi=rects, output_chroma_format=444, stack=True)
    o420 = small_store.render(index=index, roi=rects, output_chroma_format=420, stack=True)
    assert tuple(o444.shape) == (7, 3, 10, 12) and tuple(o420["y"].shape) == (7, 10, 12)
    assert tuple(o420["u"].shape) == tuple(o420["v"].shape) == (7, 5, 6)
    for j, (i, r) in enumerate(zip(index, rects)):
        _same(o444[j], small_ref[(8, 444)][i], r, 444, "stacked %d" % j)
        _same({k: v[j] for k, v in o420.items()}, small_ref[(8, 420)][i], r, 420, "stacked %d" % j)
    with pytest.raises(ValueError):
        small_store.render(index=index, roi=[(0, 0, 8, 8)] * 6 + [(0, 0, 9, 8)], stack=True)


def test_store_does_not_alias_the_streams_or_the_build_workspace(small, small_ref, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    streams = [bytes(bytearray(s)) for s in small]  # this test's own copies
    _, need = decode.decode_batch_geometry(streams)
    nstore, nws = C.c_size_t(0), C.c_size_t(0)
    keep, sp, ln = decode._marshal(streams)
    decode.check(decode._bind_latents().ccmi_latents_plan(sp, ln, 3, I16, C.byref(nstore), None, C.byref(nws)))
    del keep, sp, ln
    ws = torch.zeros(max(nws.value, 256), dtype=torch.uint8, device="cuda")
    st = decode.LatentStore(streams, dtype=torch.int16, workspace=ws)
    ws.fill_(0xA5)
    del streams
    rect = (4, 2, 20, 15)
    a = st.render(index=[0, 1, 2], roi=rect, output_chroma_format=420)
    assert decode.last_arm_flags() == []  # a render runs no ARM
    t = decode.last_timing()
    assert t["download"] == 0 and t["ups_syn_out"] > 0 and t["arm_cabac"] > 0  # [1] is the unpack here
    mid = decode.decode_batch_tensors(small, output_chroma_format=420)
    assert len(decode.last_arm_flags()) == 3
    b = st.render(index=[0, 1, 2], roi=rect, output_chroma_format=420)
    assert decode.last_arm_flags() == []
    for i in range(3):
        _same(a[i], small_ref[(8, 420)][i], rect, 420, "before")
        _same(b[i], small_ref[(8, 420)][i], rect, 420, "after")
        _same(mid[i], small_ref[(8, 420)][i], (0, 0, SMALL[i][1], SMALL[i][0]), 420, "decode_batch_tensors between")
    # errors: nothing is written, the message names the frame
    with pytest.raises(decode.CcmiError) as e:
        st.render(index=[0, 3])
    assert "frame 1" in str(e.value)
    with pytest.raises(decode.CcmiError) as e:
        st.render(index=[1, 0], roi=[(0, 0, 8, 8), (30, 20, 8, 8)])
    assert "frame 1" in str(e.value)
    with pytest.raises(decode.CcmiError):
        st.render(index=[0], workspace=torch.empty(256, dtype=torch.uint8, device="cuda"))
    st.close()
    with pytest.raises(ValueError):
        st.render()


def test_wide_form_streams(gpu, ccmi_lib):
    """The ten streams of tests/golden/cool_synth build at int32 and their whole-frame render has
    the reference decoder's md5; at int16 the streams that carry the +20,000 / -40,000 latents
    fail with NARROW (-40,000 does not fit) and the others build."""
    import torch
    import ccmi
    from ccmi import decode
    names = sorted(S.CASES)
    data = [(S.SYNTH / f"{n}.cool").read_bytes() for n in names]
    pinned = json.loads((GOLDEN / "synth_md5.json").read_text())["streams"]
    st = decode.LatentStore(data, dtype=torch.int32)
    flags = st.arm_flags  # the build's; the constructor's geometry pass has cleared the thread's record since
    assert decode.last_arm_flags() == []
    assert [f & ~NARROW for f in flags] == [S.CASES[n][5] for n in names] and not any(f & NARROW for f in flags)
    outs = st.render(workspace=_filled_ws(st, 0xA5))
    for n, o in zip(names, outs):
        yuv = b"".join(_np(o[k]).tobytes() for k in "yuv")
        assert hashlib.md5(yuv).hexdigest() == pinned[n]["md5"], n
    st.close()
    with pytest.raises(decode.CcmiError) as e:
        decode.LatentStore(data, dtype=torch.int16)
    assert e.value.code == ccmi.ERR_UNSUPPORTED
    flags = decode.last_arm_flags()
    assert [bool(f & NARROW) for f in flags] == [S.CASES[n][2] for n in names], flags
    rest = [d for n, d in zip(names, data) if not S.CASES[n][2]]
    st = decode.LatentStore(rest, dtype=torch.int16)
    assert len(st) == len(rest) and st.dtype == torch.int16
    outs = st.render()
    for n, o in zip([n for n in names if not S.CASES[n][2]], outs):
        assert hashlib.md5(b"".join(_np(o[k]).tobytes() for k in "yuv")).hexdigest() == pinned[n]["md5"], n
    st.close()
