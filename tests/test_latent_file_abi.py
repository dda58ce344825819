"""Latent files (ccmi_latents_file_head / _export_plan / _export / _import_plan / _import): the
host side.  META is written by tests/latent_file_ref.py from encode.parse's facts of the committed
streams; every handle is plan-only and no HIP call may be reached (CPU hosts have no HIP device:
a call that got as far as the runtime would return CCMI_ERR_HIP)."""
import copy
import ctypes as C
import struct

import numpy as np
import pytest

import latent_file_ref as F
from test_latent_seg_abi import COOL, I8, I16, I32, NAMES, SEG, _args, _fields

U16 = 1


@pytest.fixture(scope="module")
def L(ccmi_lib):
    from ccmi import decode
    return decode._bind()


@pytest.fixture(scope="module")
def data():
    return [(COOL / n).read_bytes() for n in NAMES]


@pytest.fixture(scope="module")
def frames(data, ccmi_lib):
    from ccmi import encode
    return [encode.parse(d) for d in data]


def _seg_words(fr):
    """Arbitrary consistent payload sizes: a third of the values, at most."""
    return [(h * w) // 3 for h, w in fr.grid_sizes]


def _streams(frames, ltype):
    return [F.stream_of_cool(fr, ltype, _seg_words(fr) if ltype == SEG else None, user_flags=2 + i)
            for i, fr in enumerate(frames)]


def _import(L, meta, first=0, count=-1, data=None, data_bytes=0, store=None, store_bytes=0, ws=None, ws_bytes=0, flags=None):
    h = C.c_void_p(0x1234)
    rc = L.ccmi_latents_import(meta, len(meta), first, count, data, data_bytes, store, store_bytes, ws, ws_bytes, None,
                               flags, C.byref(h))
    return rc, h


def _decode_handle(L, data, ltype):
    import ccmi
    h = C.c_void_p(None)
    keep, sp, ln = _args(data)
    assert L.ccmi_latents_decode(sp, ln, len(data), ltype, None, 0, None, 0, None, C.byref(h)) == 0, ccmi.last_error()
    return h


def _all_plans(L, h, index, rects):
    """Every render plan of the handle for these frames, as comparable lists."""
    import ccmi
    from ccmi import decode as D
    m = len(index)
    idx = (C.c_int * m)(*index)
    arr = None if rects is None else (D.Rect * m)(*[D.Rect(*r) for r in rects])
    fmt = D.TensorFmt(elem=D.ELEM_F32, colour=D.COLOUR_RGB)
    for c in range(3):
        fmt.scale[c] = 1.0
    rs = D.Resample(out_w=24, out_h=16, filter=D.FILTER_TRIANGLE)
    mat = np.ascontiguousarray(np.broadcast_to(D.affine_matrix((16, 24), (100.0, 60.0), 0.3, 0.5), (m, 2, 3)))
    wp = D.Warp(out_w=24, out_h=16, pad=D.PAD_FILL, matrix=mat.ctypes.data)
    out = []

    def take(rc, geom, info, need, window=None):
        assert rc == 0, ccmi.last_error()
        out.append(([_fields(g) for g in geom], [_fields(i) for i in info], need.value,
                    None if window is None else [_fields(w) for w in window]))
    geom, info, need = (D.FrameGeom * m)(), (D.RoiInfo * m)(), C.c_size_t(0)
    take(L.ccmi_latents_render_plan(h, idx, m, arr, 0, 0, U16, geom, info, C.byref(need)), geom, info, need)
    geom, info, need = (D.FrameGeom * m)(), (D.RoiInfo * m)(), C.c_size_t(0)
    take(L.ccmi_latents_render_fmt_plan(h, idx, m, arr, 0, 0, C.byref(fmt), geom, info, C.byref(need)), geom, info, need)
    geom, info, need = (D.FrameGeom * m)(), (D.RoiInfo * m)(), C.c_size_t(0)
    take(L.ccmi_latents_render_rs_plan(h, idx, m, arr, 0, 0, C.byref(fmt), C.byref(rs), geom, info, C.byref(need)), geom,
         info, need)
    geom, info, need, window = (D.FrameGeom * m)(), (D.RoiInfo * m)(), C.c_size_t(0), (D.Rect * m)()
    take(L.ccmi_latents_render_warp_plan(h, idx, m, 0, 444, C.byref(fmt), C.byref(wp), geom, info, window, C.byref(need)),
         geom, info, need, window)
    return out


@pytest.mark.parametrize("ltype", [I8, I16, I32])
def test_plan_only_import_equals_plan_only_decode(ltype, L, data, frames):
    import ccmi
    meta = F.write_meta(_streams(frames, ltype))
    n = len(data)
    # the head alone
    ns, nmeta, nfile = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    assert L.ccmi_latents_file_head(meta[:64], 64, C.byref(ns), C.byref(nmeta), C.byref(nfile)) == 0, ccmi.last_error()
    ref = F.read_meta(meta)
    assert (ns.value, nmeta.value, nfile.value) == (n, len(meta), ref["data_off"] + ref["data_bytes"])
    want = _decode_handle(L, data, ltype)
    flags = (C.c_uint32 * n)()
    rc, got = _import(L, meta, flags=flags)
    assert rc == 0 and got.value, ccmi.last_error()
    try:
        assert list(flags) == [2, 3, 4]
        assert L.ccmi_latents_count(got) == L.ccmi_latents_count(want) == n
        for i in range(n):
            a, b = (C.c_int(-1), C.c_size_t(0)), (C.c_int(-2), C.c_size_t(1))
            assert L.ccmi_latents_stream_info(got, i, C.byref(a[0]), C.byref(a[1])) == 0
            assert L.ccmi_latents_stream_info(want, i, C.byref(b[0]), C.byref(b[1])) == 0
            assert (a[0].value, a[1].value) == (b[0].value, b[1].value) == (ltype, ref["streams"][i]["part_bytes"])
        whole = ([0, 1, 2], None)
        region = ([2, 0, 1, 1], [(1600, 800, 256, 256), (2, 4, 66, 34), (512, 232, 256, 256), (0, 0, 1280, 720)])
        for index, rects in (whole, region):
            assert _all_plans(L, got, index, rects) == _all_plans(L, want, index, rects)
        # import_plan: the DATA range and the store bytes of every sub-range
        for first, count in ((0, -1), (1, 2), (2, 1), (1, -1), (0, 1)):
            off, nb, ws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(7)
            m = n - first if count < 0 else count
            each = (C.c_size_t * m)()
            assert L.ccmi_latents_import_plan(meta, len(meta), first, count, C.byref(off), C.byref(nb), each,
                                              C.byref(ws)) == 0, ccmi.last_error()
            parts = [s["part_bytes"] for s in ref["streams"]]
            assert off.value == ref["data_off"] + sum(parts[:first]) and list(each) == parts[first: first + m]
            assert nb.value == sum(parts[first: first + m]) and ws.value % 256 == 0 and ws.value > 0
            rc, sub = _import(L, meta, first, count)
            assert rc == 0, ccmi.last_error()
            one = _decode_handle(L, data[first: first + m], ltype)
            try:
                assert L.ccmi_latents_count(sub) == m
                index = list(range(m))[::-1]
                rects = [(2, 4, 66, 34)] * m
                assert _all_plans(L, sub, index, rects) == _all_plans(L, one, index, rects)
            finally:
                L.ccmi_latents_free(sub)
                L.ccmi_latents_free(one)
        # plan-only stays plan-only
        out, cap, idx = (C.c_void_p * 1)(0x1000), (C.c_size_t * 1)(1 << 20), (C.c_int * 1)(0)
        assert L.ccmi_latents_render(got, idx, 1, None, out, cap, 0, 0, 0, None, 0, None) == ccmi.ERR_ARG
        assert "plan-only" in ccmi.last_error()
    finally:
        L.ccmi_latents_free(got)
        L.ccmi_latents_free(want)


def test_plan_only_import_of_seg_streams(L, data, frames):
    """A SEG file: the render plans are those of the streams (the storage type does not enter a
    plan), the type and bytes are the record's."""
    import ccmi
    streams = _streams(frames, SEG)
    meta = F.write_meta(streams)
    rc, got = _import(L, meta)
    assert rc == 0, ccmi.last_error()
    want = _decode_handle(L, data, I16)
    try:
        for i, s in enumerate(streams):
            t, nb = C.c_int(-1), C.c_size_t(0)
            assert L.ccmi_latents_stream_info(got, i, C.byref(t), C.byref(nb)) == 0
            assert (t.value, nb.value) == (SEG, s["part_bytes"])
        index, rects = [1, 0, 2], [(512, 232, 256, 256), (2, 4, 66, 34), (1600, 800, 256, 256)]
        assert _all_plans(L, got, index, rects) == _all_plans(L, want, index, rects)
        # and its export plan gives the file back
        a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        assert L.ccmi_latents_export_plan(got, None, 3, C.byref(a), C.byref(b), C.byref(c)) == 0, ccmi.last_error()
        ref = F.read_meta(meta)
        assert (a.value, b.value) == (len(meta), ref["data_off"] + ref["data_bytes"])
    finally:
        L.ccmi_latents_free(got)
        L.ccmi_latents_free(want)


def test_export_plan(L, data, frames):
    import ccmi
    h = _decode_handle(L, data, I16)
    try:
        streams = _streams(frames, I16)
        for index in (None, [2, 0, 2, 1, 2]):
            pick = streams if index is None else [streams[i] for i in index]
            meta = F.write_meta(pick)
            ref = F.read_meta(meta)
            m = len(pick)
            idx = None if index is None else (C.c_int * m)(*index)
            a, b, ws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
            assert L.ccmi_latents_export_plan(h, idx, m, C.byref(a), C.byref(b), C.byref(ws)) == 0, ccmi.last_error()
            assert (a.value, b.value) == (len(meta), ref["data_off"] + ref["data_bytes"])
            assert ws.value >= ref["data_bytes"] and ws.value % 256 == 0
        a = C.c_size_t(0)
        assert L.ccmi_latents_export_plan(None, None, 1, C.byref(a), None, None) == ccmi.ERR_ARG
        assert L.ccmi_latents_export_plan(h, None, 2, C.byref(a), None, None) == ccmi.ERR_ARG
        bad = (C.c_int * 1)(3)
        assert L.ccmi_latents_export_plan(h, bad, 1, C.byref(a), None, None) == ccmi.ERR_ARG and "index 3" in ccmi.last_error()
        # the export itself needs the latents
        buf = C.create_string_buffer(1 << 20)
        assert L.ccmi_latents_export(h, None, 3, None, buf, 1 << 20, None, 0, None) == ccmi.ERR_ARG
        assert "plan-only" in ccmi.last_error()
    finally:
        L.ccmi_latents_free(h)


def _set(streams, i, **kw):
    out = copy.deepcopy(streams)
    for k, v in kw.items():
        if k in F.HDR:
            out[i]["hdr"][k] = v
        else:
            out[i][k] = v
    return out


def _refused(L, meta, code, *words, **kw):
    import ccmi
    rc, h = _import(L, meta, **kw)
    msg = ccmi.last_error()
    assert rc == code and h.value is None, (rc, msg)
    for w in words:
        assert w in msg, msg
    off = C.c_size_t(0)
    if not kw:
        assert L.ccmi_latents_import_plan(meta, len(meta), 0, -1, C.byref(off), None, None, None) == code


def test_refusals(L, frames):
    import ccmi
    BS, ARG = ccmi.ERR_BITSTREAM, ccmi.ERR_ARG
    base = _streams(frames, SEG)
    good = F.write_meta(base)
    rc, h = _import(L, good)
    assert rc == 0
    L.ccmi_latents_free(h)
    _refused(L, F.write_meta(base, magic=b"CCMILAT2"), BS, "magic")
    _refused(L, F.write_meta(base, version=2), BS, "version 2")
    _refused(L, F.write_meta(base, n_streams=0), BS, "n_streams 0")
    for n in range(len(good)):  # truncated at every length
        rc, h = _import(L, good[:n])
        assert rc == BS and h.value is None, (n, rc, ccmi.last_error())
    _refused(L, F.write_meta(base, index_bytes=len(good) - 64 - 8), BS)
    _refused(L, F.write_meta(base, index_bytes=len(good) - 64 + 8) + b"\0" * 8, BS)
    _refused(L, F.write_meta(base, data_off=F.align(len(good), 256) + 8), BS, "data_off")
    _refused(L, F.write_meta(base, data_off=F.align(len(good), 256) + 256), BS, "data_off")
    short = _set(base, 1, record_bytes=len(F.record(base[1])) - 8)
    _refused(L, F.write_meta(short), BS, "stream 1")
    _refused(L, F.write_meta(_set(base, 2, type=4)), BS, "stream 2", "latent_type 4")
    nine = _set(base, 1, n_layers=9, lat_n=[1] * 9, seg_words=[0] * 9)
    _refused(L, F.write_meta(nine), BS, "stream 1", "layer count 9")
    _refused(L, F.write_meta(_set(base, 0, layers=[(3, 1, 0, 0)] * 17)), BS, "stream 0", "layer count 17")
    even = _set(base, 2, layers=[(a, 2 if k == 0 else b, c, d) for k, (a, b, c, d) in enumerate(base[2]["layers"])])
    _refused(L, F.write_meta(even), BS, "stream 2", "kernel size 2")
    for h_, w_ in ((1 << 16, 1 << 16), (0x7FFFFFFF, 0x7FFFFFFF), (-1, 4)):
        _refused(L, F.write_meta(_set(base, 1, h=h_, w=w_)), BS, "stream 1", "frame size")
    _refused(L, F.write_meta(_set(base, 1, part_bytes=base[1]["part_bytes"] + 256)), BS, "stream 1", "part_bytes")
    _refused(L, F.write_meta(_set(base, 1, part_bytes=base[1]["part_bytes"] - 256)), BS, "stream 1", "part_bytes")
    big = _set(base, 2, seg_words=[(1 << 29) + 64] + base[2]["seg_words"][1:])
    big[2]["part_bytes"] = F.part_ranges(SEG, big[2]["hdr"], big[2]["layers"], big[2]["lat_n"], big[2]["seg_words"])[1]
    _refused(L, F.write_meta(big), BS, "stream 2", "grid 0", "seg_words")
    over = _set(base, 0, seg_words=[base[0]["hdr"]["h"] * base[0]["hdr"]["w"] + 1] + base[0]["seg_words"][1:])
    over[0]["part_bytes"] = F.part_ranges(SEG, over[0]["hdr"], over[0]["layers"], over[0]["lat_n"], over[0]["seg_words"])[1]
    _refused(L, F.write_meta(over), BS, "stream 0", "grid 0", "seg_words")
    _refused(L, F.write_meta(_set(base, 1, blend=[5])), BS, "stream 1", "blend")
    _refused(L, F.write_meta(_set(base, 1, n_branches=2)), BS, "stream 1", "blend")
    # seg_words of a typed stream
    typed = _streams(frames, I16)
    _refused(L, F.write_meta(_set(typed, 1, seg_words=[4] + [0] * (typed[1]["hdr"]["n_layers"] - 1))), BS, "stream 1", "grid 0")
    # one flipped bit anywhere in the INDEX, index_sum left alone
    for at in range(64, len(good), 7):
        bad = bytearray(good)
        bad[at] ^= 1 << (at % 8)
        _refused(L, bytes(bad), BS, "index_sum")
    # arguments
    for first, count in ((-1, 1), (3, 1), (0, 4), (2, 2), (0, 0), (1, 3)):
        _refused(L, good, ARG, "streams", first=first, count=count)
    h = C.c_void_p(0x1234)
    assert L.ccmi_latents_import(None, 64, 0, -1, None, 0, None, 0, None, 0, None, None, C.byref(h)) == ARG and h.value is None
    assert L.ccmi_latents_import(good, len(good), 0, -1, None, 0, None, 0, None, 0, None, None, None) == ARG
    # a store with no GPU behind it: every argument fault is found before a HIP call
    need = sum(s["part_bytes"] for s in base)
    host = C.create_string_buffer(16)
    hp = C.addressof(host)
    _refused(L, good, ARG, "256-byte aligned", data=hp, data_bytes=need, store=0x10001, store_bytes=need)
    _refused(L, good, ARG, "store of", str(need), data=hp, data_bytes=need, store=0x10000, store_bytes=need - 1)
    _refused(L, good, ARG, "data of", str(need), data=hp, data_bytes=need - 1, store=0x10000, store_bytes=need)
    _refused(L, good, ARG, "go together", data=hp, data_bytes=need)
    _refused(L, good, ARG, "go together", store=0x10000, store_bytes=need)
    _refused(L, good, ARG, "workspace", data=hp, data_bytes=need, store=0x10000, store_bytes=need, ws=0x20000, ws_bytes=16)
    _refused(L, good, ARG, "workspace", data=hp, data_bytes=need, store=0x10000, store_bytes=need, ws=0x20001,
             ws_bytes=1 << 30)


def test_file_head_and_symbols(L, frames):
    import ccmi
    good = F.write_meta(_streams(frames, I8))
    n = C.c_int(0)
    assert L.ccmi_latents_file_head(good, 63, C.byref(n), None, None) == ccmi.ERR_BITSTREAM
    assert L.ccmi_latents_file_head(None, 64, C.byref(n), None, None) == ccmi.ERR_ARG
    assert L.ccmi_latents_file_head(good, 64, None, None, None) == 0
    bad = bytearray(good)
    bad[56] = 1
    assert L.ccmi_latents_file_head(bytes(bad), 64, C.byref(n), None, None) == ccmi.ERR_BITSTREAM
    for name in ("ccmi_latents_file_head", "ccmi_latents_export_plan", "ccmi_latents_export", "ccmi_latents_import_plan",
                 "ccmi_latents_import"):
        assert name in ccmi.EXPORTED and hasattr(L, name)
    assert L.ccmi_version() >= 101


def test_committed_meta_blocks_are_the_reference_writers(L, frames):
    """tests/golden/latent_meta/*.meta, the inputs of tools/latents_file_san.cpp: what the reference
    writer makes of the committed streams today, and what the library accepts."""
    import ccmi
    golden = COOL.parent / "latent_meta"
    for name, ltype in (("i8", I8), ("i16", I16), ("i32", I32), ("seg", SEG)):
        meta = (golden / (name + ".meta")).read_bytes()
        assert meta == F.write_meta(_streams(frames, ltype)), name
        rc, h = _import(L, meta)
        assert rc == 0, ccmi.last_error()
        L.ccmi_latents_free(h)


def test_file_info_needs_no_gpu(L, frames, tmp_path):
    import torch
    from ccmi import decode
    streams = _streams(frames, I16)
    meta = F.write_meta(streams)
    p = tmp_path / "x.cclat"
    p.write_bytes(meta)  # META is all file_info reads
    info = decode.LatentStore.file_info(p)
    assert info["n_streams"] == 3 and info["meta_bytes"] == len(meta)
    ref = F.read_meta(meta)
    assert info["file_bytes"] == ref["data_off"] + ref["data_bytes"]
    for s, r in zip(info["streams"], ref["streams"]):
        assert (s["width"], s["height"]) == (r["hdr"]["w"], r["hdr"]["h"])
        assert s["dtype"] == torch.int16 and s["nbytes"] == r["part_bytes"] and s["arm_flags"] == r["user_flags"]
