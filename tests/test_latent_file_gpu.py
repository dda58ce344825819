"""Latent files on the GPU: ccmi_latents_export / ccmi_latents_import and LatentStore.save / load /
file_info.  Every comparison is bitwise: the file form, the checksums and the renders are integer
or already-pinned contracts.  The file is read and written by tests/latent_file_ref.py, a numpy
restatement of the contract in include/ccmi.h; the streams, the stores and the reference planes are
those of tests/test_latent_seg_gpu.py (partial segments, grids under one 16-byte group, an empty
grid, all six width codes)."""
import ctypes as C

import numpy as np
import pytest

import latent_file_ref as F
from test_latent_seg_gpu import (I8, I16, I32, N16, SEG, WIDE, _reference_images, _wide_rects,  # noqa: F401
                                 compacted, latents, planes, source, streams)
from test_latent_store_gpu import _filled_ws, _np, _same

pytestmark = pytest.mark.gpu
GUARD = 256


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _build(data, ltype, fill):
    """ccmi_latents_decode into a store pre-filled with `fill`.  -> (handle, store tensor, bytes)"""
    import torch
    from ccmi import decode
    L = decode._bind()
    n = len(data)
    keep, sp, ln = decode._marshal(data)
    nstore, nws = C.c_size_t(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_plan(sp, ln, n, ltype, C.byref(nstore), None, C.byref(nws)))
    store = torch.full((nstore.value + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws = torch.full((max(nws.value, 256),), fill, dtype=torch.uint8, device="cuda")
    h = C.c_void_p(None)
    decode.check(L.ccmi_latents_decode(sp, ln, n, ltype, store.data_ptr(), nstore.value, ws.data_ptr(), ws.numel(),
                                       _stream(), C.byref(h)))
    torch.cuda.synchronize()
    return h, store, nstore.value


def _compact(h_src, fill):
    import torch
    from ccmi import decode
    L = decode._bind()
    bound, nws, exact = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_compact_plan(h_src, C.byref(bound), C.byref(nws)))
    ws = torch.full((max(nws.value, 256),), fill, dtype=torch.uint8, device="cuda")
    decode.check(L.ccmi_latents_compact_measure(h_src, ws.data_ptr(), ws.numel(), _stream(), C.byref(exact), None))
    store = torch.full((exact.value + GUARD,), fill, dtype=torch.uint8, device="cuda")
    h = C.c_void_p(None)
    decode.check(L.ccmi_latents_compact(h_src, store.data_ptr(), exact.value, ws.data_ptr(), ws.numel(), _stream(),
                                        C.byref(h)))
    torch.cuda.synchronize()
    return h, store, exact.value


def _export(h, index=None, flags=None, fill=0xA5):
    """ccmi_latents_export_plan / _export: workspace and host buffer pre-filled.  -> the file's bytes"""
    import torch
    from ccmi import decode
    L = decode._bind()
    m = L.ccmi_latents_count(h) if index is None else len(index)
    idx = None if index is None else (C.c_int * m)(*index)
    fl = None if flags is None else (C.c_uint32 * m)(*flags)
    nmeta, nfile, nws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_export_plan(h, idx, m, C.byref(nmeta), C.byref(nfile), C.byref(nws)))
    ws = torch.full((max(nws.value, 256),), fill, dtype=torch.uint8, device="cuda")
    buf = np.full(nfile.value + GUARD, fill, dtype=np.uint8)
    decode.check(L.ccmi_latents_export(h, idx, m, fl, buf.ctypes.data, nfile.value, ws.data_ptr(), ws.numel(), _stream()))
    assert (buf[nfile.value:] == fill).all(), "the export wrote past file_bytes"
    return buf[: nfile.value].tobytes()


def _import(file, first=0, count=-1, fill=0xA5):
    """ccmi_latents_file_head / _import_plan / _import of streams [first, first + count): the store
    pre-filled, 256 guard bytes behind it.  -> (rc, handle, store tensor, data bytes, user flags)"""
    import torch
    from ccmi import decode
    L = decode._bind()
    n, nmeta = C.c_int(0), C.c_size_t(0)
    decode.check(L.ccmi_latents_file_head(file[:64], 64, C.byref(n), C.byref(nmeta), None))
    meta = file[: nmeta.value]
    off, nb, nws = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = L.ccmi_latents_import_plan(meta, len(meta), first, count, C.byref(off), C.byref(nb), None, C.byref(nws))
    if rc:
        return rc, C.c_void_p(None), None, 0, []
    m = n.value - first if count < 0 else count
    data = np.frombuffer(file, dtype=np.uint8)[off.value: off.value + nb.value].copy()
    store = torch.full((nb.value + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws = torch.full((max(nws.value, 256),), fill, dtype=torch.uint8, device="cuda")
    flags, h = (C.c_uint32 * m)(), C.c_void_p(0x1234)
    rc = L.ccmi_latents_import(meta, len(meta), first, count, data.ctypes.data, nb.value, store.data_ptr(), nb.value,
                               ws.data_ptr(), ws.numel(), _stream(), flags, C.byref(h))
    torch.cuda.synchronize()
    assert (_np(store[nb.value:]) == fill).all(), "the import wrote past data_bytes"
    return rc, h, store, nb.value, list(flags)


def _adopt(h, store, flags):
    from ccmi import decode
    st = decode.LatentStore.__new__(decode.LatentStore)
    st._adopt(h, [store], flags)
    return st


def _each(h):
    from ccmi import decode
    L = decode._bind()
    out = []
    for i in range(L.ccmi_latents_count(h)):
        t, nb = C.c_int(-1), C.c_size_t(0)
        decode.check(L.ccmi_latents_stream_info(h, i, C.byref(t), C.byref(nb)))
        out.append((t.value, nb.value))
    return out


def _check_file(file, data, h, store, flags):
    """The exported file through the reference reader: HEAD / INDEX against encode.parse's facts and
    ccmi_latents_stream_info, DATA against the device store under the reference's mask (the reader
    has checked that every other byte is 0 and both kinds of checksum)."""
    from ccmi import encode
    f = F.read_file(file)
    each = _each(h)
    assert f["n_streams"] == len(data) == len(each)
    dev, pos = _np(store), 0
    for i, (s, b, (t, nb)) in enumerate(zip(f["streams"], data, each)):
        want = F.stream_of_cool(encode.parse(b), t)
        for k in ("hdr", "layers", "lat_n", "blend"):
            assert s[k] == want[k] or [tuple(x) for x in s[k]] == want[k], (i, k, s[k], want[k])
        assert (s["type"], s["part_bytes"], s["user_flags"]) == (t, nb, flags[i]), i
        if t != SEG:
            assert s["seg_words"] == [0] * len(s["lat_n"])
        part = np.frombuffer(s["part"], dtype=np.uint8)
        bad = np.flatnonzero((part != dev[pos: pos + nb]) & s["mask"])
        assert bad.size == 0, ("stream %d: %d bytes differ from the store, the first at %d" % (i, bad.size, int(bad[0])))
        pos += nb
    return f


@pytest.mark.parametrize("ltype", [I8, I16, I32])
def test_export_is_the_contract(ltype, streams, latents, gpu, ccmi_lib):
    """Typed stores built over 0xA5 and over 0x5A export the same file; so do their compactions; the
    file is the store under the defined-byte mask and 0 elsewhere."""
    from ccmi import decode
    L = decode._bind()
    keep = {I8: [0, 1, 2, 4, 5], I16: list(range(N16)), I32: list(range(len(streams)))}[ltype]
    data = [streams[i][1] for i in keep]
    flags = [3 + i for i in range(len(data))]
    files, seg_files = [], []
    for fill in (0xA5, 0x5A):
        h, store, nbytes = _build(data, ltype, fill)
        try:
            before = _np(store).copy()
            files.append(_export(h, flags=flags, fill=fill))
            assert np.array_equal(_np(store), before), "the export wrote to the source store"
            f = _check_file(files[-1], data, h, store, flags)
            # the grids are the reference's: decode_latents at the store's element type
            for s, i in zip(f["streams"], keep):
                for name, off, nb in s["ranges"]:
                    if name.startswith("grid"):
                        want = np.asarray(latents[i][int(name[4:])]).reshape(-1).astype(F.ELEM[ltype])
                        assert s["part"][off: off + nb] == want.tobytes(), (i, name)
            if ltype != I8:
                hc, cstore, _ = _compact(h, fill)
                try:
                    seg_files.append(_export(hc, flags=flags, fill=fill))
                    _check_file(seg_files[-1], data, hc, cstore, flags)
                finally:
                    L.ccmi_latents_free(hc)
        finally:
            L.ccmi_latents_free(h)
    assert files[0] == files[1], "the file depends on what the store's padding held"
    if seg_files:
        assert seg_files[0] == seg_files[1]


def _ref_seg_file(data, lats, src_store, src_each, flags):
    """The SEG file of these streams written by the reference writer: grids from decode_latents
    through latent_seg_ref.pack_grid, the networks' integers from the source store."""
    from ccmi import encode
    out = []
    for b, (img, _, grids), fl in zip(data, _reference_images(data, lats, src_store, src_each), flags):
        words = [0 if g is None else len(g[1]) for g in grids]
        s = F.stream_of_cool(encode.parse(b), SEG, words, user_flags=fl)
        del s["part_bytes"], s["part_sum"]
        s["part"] = img
        out.append(s)
    return F.write_file(out), out


@pytest.fixture(scope="module")
def ref_file(streams, latents, source, gpu, ccmi_lib):
    data = [b for _, b, _ in streams[:N16]]
    return _ref_seg_file(data, latents[:N16], source._store, source.stream_nbytes, list(range(10, 10 + N16)))


def test_compactions_of_i16_and_i32_export_the_reference_file(streams, ref_file, gpu, ccmi_lib):
    from ccmi import decode
    L = decode._bind()
    data = [b for _, b, _ in streams[:N16]]
    flags = list(range(10, 10 + N16))
    got = []
    for ltype, fill in ((I16, 0xA5), (I32, 0x5A)):
        h, store, _ = _build(data, ltype, fill)
        hc, cstore, _ = _compact(h, fill)
        L.ccmi_latents_free(h)
        got.append(_export(hc, flags=flags, fill=fill))
        L.ccmi_latents_free(hc)
    assert got[0] == got[1], "compactions from I16 and I32 export different files"
    assert got[0] == ref_file[0], "the exported file is not the reference writer's"


def test_import_is_the_contract(streams, latents, planes, compacted, ref_file, gpu, ccmi_lib):
    """The reference writer's file imported: the store is DATA, the guard stays, the renders and the
    latents are the compacted store's."""
    import ccmi
    import torch
    file, recs = ref_file
    ref = F.read_file(file)
    rc, h, store, nb, flags = _import(file)
    assert rc == 0 and h.value, ccmi.last_error()
    # the thread's record of the last call: no ARM ran, no tail ran, upload and checksum + verify timed
    from ccmi import decode
    tm = decode.last_timing()
    assert decode.last_arm_flags() == [] and decode.last_tail_groups() == (0, 0)
    assert tm["upload"] > 0 and tm["arm_cabac"] > 0 and tm["ups_syn_out"] == 0 and tm["download"] == 0
    assert flags == list(range(10, 10 + N16)) and nb == ref["data_bytes"]
    assert _np(store[:nb]).tobytes() == file[ref["data_off"]:], "the store is not the DATA range"
    st = _adopt(h, store, flags)
    try:
        assert st.stream_dtypes == ["seg"] * N16 and st.stream_nbytes == compacted.stream_nbytes
        assert st.geometry == compacted.geometry
        for bitdepth, chroma in ((8, 420), (8, 444), (10, 420), (10, 444)):
            kw = dict(output_bitdepth=bitdepth, output_chroma_format=chroma)
            want = compacted.render(**kw)
            for fill in (0xA5, 0x5A):
                outs = st.render(workspace=_filled_ws(st, fill, **kw), **kw)
                for i, (o, w) in enumerate(zip(outs, want)):
                    hh, ww = streams[i][2]
                    _same(o, planes[(bitdepth, chroma)][i], (0, 0, ww, hh), chroma, "fill %#x" % fill)
                    for k in (("y", "u", "v") if isinstance(o, dict) else range(len(o))):
                        assert torch.equal(o[k], w[k]), (bitdepth, chroma, i, k)
        rects = _wide_rects()
        kw = dict(index=[3] * len(rects), roi=rects, output_bitdepth=8, output_chroma_format=444)
        want = compacted.render(**kw)
        for fill in (0xA5, 0x5A):
            outs = st.render(workspace=_filled_ws(st, fill, **kw), **kw)
            for r, o, w in zip(rects, outs, want):
                assert torch.equal(o, w), (r, fill)
        for i in range(N16):
            for l, (g, w) in enumerate(zip(st.latents(i), latents[i])):
                assert np.array_equal(_np(g).reshape(-1), np.asarray(w).reshape(-1)), (i, l)
        # the class-D stream with the empty grid: no bytes in the file, zeros in the render's planes
        empty = [l for l, nbytes in enumerate(recs[5]["lat_n"]) if nbytes == 0]
        assert empty and all(not n.endswith(str(l)) for l in empty for n, _, _ in ref["streams"][5]["ranges"])
        for l in empty:
            assert not _np(st.latents(5)[l]).any()
    finally:
        st.close()


def test_round_trip_through_python(streams, source, compacted, tmp_path, gpu, ccmi_lib):
    import math
    import torch
    from ccmi import decode
    for name, st in (("i16", source), ("seg", compacted)):
        p = tmp_path / (name + ".cclat")
        nfile = st.save(p)
        assert p.stat().st_size == nfile and sorted(x.name for x in tmp_path.iterdir() if x.name.startswith(name)) == [p.name]
        info = decode.LatentStore.file_info(p)
        assert info["n_streams"] == len(st) and info["file_bytes"] == nfile
        assert [{k: s[k] for k in st.geometry[0]} for s in info["streams"]] == st.geometry
        assert [s["dtype"] for s in info["streams"]] == st.stream_dtypes
        assert [s["nbytes"] for s in info["streams"]] == st.stream_nbytes
        assert [s["arm_flags"] for s in info["streams"]] == st.arm_flags
        ld = decode.LatentStore.load(p)
        try:
            assert len(ld) == len(st) and ld.geometry == st.geometry and ld.stream_dtypes == st.stream_dtypes
            assert ld.stream_nbytes == st.stream_nbytes and ld.arm_flags == st.arm_flags
            index = [3, 0, 4, 5, 1, 2]
            kw = dict(index=index, roi=[(60, 2, 70, 20), (0, 0, 36, 20), (64, 32, 200, 100), (0, 0, 416, 240), (2, 2, 40, 30),
                                        (2, 2, 30, 18)],
                      size=(24, 24), dtype=torch.bfloat16, colour="rgb", mean=(0.4, 0.5, 0.6), std=(0.2, 0.3, 0.25))
            a, b = st.render_model(**kw), ld.render_model(**kw)
            assert tuple(a.shape) == (6, 3, 24, 24) and torch.equal(a.view(torch.int16), b.view(torch.int16))
            kw.pop("size")
            kw.update(index=[3, 3], roi=[(60, 2, 70, 20)] * 2)
            a, b = st.render_model(**kw), ld.render_model(**kw)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            kw.pop("roi")
            mats = np.stack([decode.affine_matrix((24, 24), (w / 2, h / 2), math.radians(20 + 10 * j), 0.8)
                             for j, (_, _, (h, w)) in enumerate(streams[i] for i in index)])
            kw.update(index=index, affine=mats, size=(24, 24), output_chroma_format=444)  # odd frame sizes
            a, b = st.render_model(**kw), ld.render_model(**kw)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            if name == "i16":
                # a loaded typed store compacts to the original's compaction: every byte of the store the
                # contract defines (the padding of a torch.empty store is anything), which is what a file holds
                c = ld.compact()
                assert c.stream_nbytes == compacted.stream_nbytes
                assert _export(c._handle()) == _export(compacted._handle())
                f = F.read_file(_export(c._handle()))
                dev = _np(c._store)
                for s in f["streams"]:
                    at = s["data_at"] - f["data_off"]
                    part = np.frombuffer(s["part"], dtype=np.uint8)
                    assert np.array_equal(part[s["mask"]], dev[at: at + s["part_bytes"]][s["mask"]])
                c.close()
        finally:
            ld.close()


def test_resharding_a_mixed_concat(streams, planes, tmp_path, gpu, ccmi_lib):
    """index = [3, 0, 3, 6] over concat(I8, SEG, I32) -> a mixed-type file; load(first=1, count=2)
    needs that DATA range only; concat of two loads equals one load."""
    import torch
    from ccmi import decode
    data = [b for _, b, _ in streams]
    a = decode.LatentStore(data[:3], dtype=torch.int8)
    b16 = decode.LatentStore(data[3:6], dtype=torch.int16)
    b = b16.compact()
    c = decode.LatentStore(data[6:], dtype=torch.int32)
    cat = decode.LatentStore.concat([a, b, c])
    index = [3, 0, 3, 6]
    p = tmp_path / "mixed.cclat"
    cat.save(p, index=index)
    f = F.read_file(p.read_bytes())
    assert [s["type"] for s in f["streams"]] == [SEG, I8, SEG, I32]
    assert f["streams"][0]["part"] == f["streams"][2]["part"]
    kw = dict(output_bitdepth=8, output_chroma_format=444)
    want = cat.render(index=index, **kw)
    for st in (a, b16, b, c, cat):
        st.close()
    # everything of DATA outside streams 1 and 2 destroyed: the load of those two does not read it
    q = tmp_path / "holes.cclat"
    raw = bytearray(p.read_bytes())
    lo, hi = f["streams"][1]["data_at"], f["streams"][2]["data_at"] + f["streams"][2]["part_bytes"]
    raw[f["data_off"]: lo] = b"\xEE" * (lo - f["data_off"])
    raw[hi:] = b"\xEE" * (len(raw) - hi)
    q.write_bytes(bytes(raw))
    mm = np.memmap(q, dtype=np.uint8, mode="r")
    assert (mm[f["data_off"]: lo] == 0xEE).all() and (mm[hi:] == 0xEE).all() and bytes(mm[lo:hi]) == bytes(raw[lo:hi])
    del mm
    part = decode.LatentStore.load(q, first=1, count=2)
    whole = decode.LatentStore.load(p)
    two = decode.LatentStore.concat([decode.LatentStore.load(p, first=0, count=1), decode.LatentStore.load(p, first=1)])
    try:
        assert part.stream_dtypes == [torch.int8, "seg"] and whole.stream_dtypes == ["seg", torch.int8, "seg", torch.int32]
        assert two.stream_dtypes == whole.stream_dtypes and two.stream_nbytes == whole.stream_nbytes
        assert two.geometry == whole.geometry and two.arm_flags == whole.arm_flags
        with pytest.raises(decode.CcmiError):
            decode.LatentStore.load(q)  # the destroyed parts do not pass their checksums
        for st, sel in ((whole, [0, 1, 2, 3]), (two, [0, 1, 2, 3]), (part, [1, 2])):
            for fill in (0xA5, 0x5A):
                outs = st.render(workspace=_filled_ws(st, fill, **kw), **kw)
                for o, k in zip(outs, sel):
                    hh, ww = streams[index[k]][2]
                    _same(o, planes[(8, 444)][index[k]], (0, 0, ww, hh), 444, "stream %d" % k)
                    assert torch.equal(o, want[k])
    finally:
        for st in (part, whole, two):
            st.close()


def _clean(s):
    return {k: s[k] for k in ("type", "user_flags", "hdr", "layers", "lat_n", "seg_words", "blend", "part")}


def _words(s, name):
    off, nb = next((o, n) for k, o, n in s["ranges"] if k == name)
    return off, np.frombuffer(s["part"], dtype="<u4", count=nb // 4, offset=off).copy()


def _put(s, off, words):
    raw = bytearray(s["part"])
    raw[off: off + 4 * len(words)] = np.asarray(words, dtype="<u4").tobytes()
    s["part"] = bytes(raw)


def test_corrupt_files_are_refused(streams, source, ref_file, gpu, ccmi_lib):
    import ccmi
    good = F.read_file(ref_file[0])

    def refused(streams_, *words, keep_sum=False):
        out = []
        for s, g in zip(streams_, good["streams"]):
            c = _clean(s)
            if keep_sum:
                c["part_sum"] = g["part_sum"]
            out.append(c)
        rc, h, store, nb, _ = _import(F.write_file(out))
        msg = ccmi.last_error()
        assert rc == ccmi.ERR_BITSTREAM and h.value is None, (rc, msg)
        for w in words:
            assert w in msg, msg

    def fresh():
        return [dict(s) for s in good["streams"]]
    # one payload bit: the checksum
    ss = fresh()
    off, w = _words(ss[3], "payload0")
    w[len(w) // 2] ^= 1 << 9
    _put(ss[3], off, w)
    refused(ss, "stream 3", "part_sum", keep_sum=True)
    # the next five carry a recomputed part_sum: only the verify kernel stands in their way
    ss = fresh()
    off, d = _words(ss[3], "desc0")
    d[5] = (d[5] & ~np.uint32(7)) | np.uint32(6)
    _put(ss[3], off, d)
    refused(ss, "stream 3", "grid 0", "width code")
    ss = fresh()
    off, d = _words(ss[3], "desc1")
    d[7] += 8
    _put(ss[3], off, d)
    refused(ss, "stream 3", "grid 1", "offset")
    ss = fresh()
    off, d = _words(ss[0], "desc0")
    d[-1] = ((ss[0]["seg_words"][0] + 5) << 3) | (int(d[-1]) & 7)
    _put(ss[0], off, d)
    refused(ss, "stream 0", "grid 0", "offset")
    ss = fresh()
    off, d = _words(ss[4], "desc0")
    j = next(j for j in range(len(d) - 1) if d[j] != d[j + 1])
    d[j], d[j + 1] = d[j + 1], d[j]
    _put(ss[4], off, d)
    refused(ss, "stream 4", "grid 0")
    # seg_words one more than the descriptors' total, inside the payload's 16-byte rounding
    ss = fresh()
    i, l = next((i, l) for i, s in enumerate(ss) for l, n in enumerate(s["seg_words"]) if n % 4)
    ss[i]["seg_words"] = list(ss[i]["seg_words"])
    ss[i]["seg_words"][l] += 1
    assert F.part_ranges(SEG, ss[i]["hdr"], ss[i]["layers"], ss[i]["lat_n"], ss[i]["seg_words"])[1] == ss[i]["part_bytes"]
    refused(ss, "stream %d" % i, "grid %d" % l, "seg_words")
    # an I16 file: one flipped bit in a grid
    from ccmi import decode
    file = _export(source._handle())
    f16 = F.read_file(file)
    ss = [dict(s) for s in f16["streams"]]
    off, nb = next((o, n) for k, o, n in ss[1]["ranges"] if k == "grid0")
    raw = bytearray(ss[1]["part"])
    raw[off + nb // 2] ^= 4
    ss[1]["part"] = bytes(raw)
    out = [dict(_clean(s), part_sum=g["part_sum"]) for s, g in zip(ss, f16["streams"])]
    rc, h, _, _, _ = _import(F.write_file(out))
    assert rc == ccmi.ERR_BITSTREAM and h.value is None and "stream 1" in ccmi.last_error()
    # and the files these were made from import
    for ok in (ref_file[0], file):
        rc, h, _, _, _ = _import(ok)
        assert rc == 0 and h.value, ccmi.last_error()
        decode._bind().ccmi_latents_free(h)
