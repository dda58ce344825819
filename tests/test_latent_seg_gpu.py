"""Compact latent stores (CCMI_LATENT_SEG: ccmi_latents_compact*, LatentStore.compact) and one
handle over many stores (ccmi_latents_concat, LatentStore.concat).

Every comparison is bitwise.  The store's bytes are compared with tests/latent_seg_ref.py, a numpy
restatement of the contract, fed with decode.decode_latents; values and samples with the code that
existed before the store, as tests/test_latent_store_gpu.py does: decode.decode_latents and the
planes of decode.decode_batch cropped in numpy.

The streams: the generated 21 x 37, 34 x 66 and generic-synthesis 21 x 37 ones of the latent store's
tests; one of 24 x 150 (rows of two full segments and 22 values; the next grid 64 + 11) whose
latents are drawn per segment from ranges that need 0, 2, 4 and 8 bits, with every width boundary
planted at a segment's first and last position, the partial segments included; two committed
class-D streams, one with an empty grid; a second 24 x 150 stream that also carries the -32769 / 32768
boundaries (it fits no int16 store and is compacted from an int32 one); and d16h0_q32 with its
-40000 / 20000 latents."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import latent_seg_ref as R
import synth_streams as S
from test_latent_store_gpu import GOLDEN, FILES, SMALL, _c_build, _c_values, _filled_ws, _generate, _np, _planes, _same

I8, I16, I32, SEG = 0, 1, 2, 3
WIDE = (24, 150)
PAIRS = [(-1, 0), (0, 1), (-2, 1), (-3, 0), (0, 2), (-8, 7), (-9, 0), (0, 8), (-128, 127), (-129, 0), (0, 128),
         (-32768, 32767)]
PAIRS32 = PAIRS + [(-32769, 0), (0, 32768)]
N16 = 6  # streams[:N16] fit int16

pytestmark = pytest.mark.gpu


def _wide_plants(pairs, seed):
    """Grids 0 (24 x 150) and 1 (12 x 75) in full, as _generate's plants."""
    rng = np.random.default_rng(seed)
    spans = [0, 1, 7, 100]  # codes 0, 2, 4, 8
    plants = []
    for grid, (h, w) in enumerate(((24, 150), (12, 75))):
        nseg = (w + 63) // 64
        g = np.zeros((h, w), dtype=np.int64)
        for r in range(h):
            planted = (r // len(pairs) + r) % nseg
            for s in range(nseg):
                c = min(64 * s + 64, w) - 64 * s
                span = spans[(r + s) % 4]
                seg = rng.integers(-span - 1, span + 1, size=c) if span else np.zeros(c, dtype=np.int64)
                if s == planted:  # values inside the pair's range, the pair at both ends
                    lo, hi = pairs[r % len(pairs)]
                    seg = rng.integers(max(lo, -2), min(hi, 1) + 1, size=c)
                    seg[0], seg[-1] = (lo, hi) if r % 2 == 0 else (hi, lo)
                g[r, 64 * s: 64 * s + c] = seg
        plants += [(grid, i, int(v)) for i, v in enumerate(g.reshape(-1))]
    return tuple(plants)


@pytest.fixture(scope="module")
def streams(gpu, ccmi_lib):
    """[(name, bytes, (h, w))]: small x 3, wide, class D x 2 (the second with an empty grid), and
    last the wide stream that needs int32."""
    from ccmi import encode
    out = [("small%d" % i, _generate(h, w, seed, generic=gen), (h, w))
           for i, ((h, w), seed, gen) in enumerate(zip(SMALL, (7, 9, 11), (False, False, True)))]
    out.append(("wide", _generate(WIDE[0], WIDE[1], 13, plants=_wide_plants(PAIRS, 150)), WIDE))
    d_files = [f for f in FILES if f.name.startswith("D-")]
    empty = [f for f in d_files if 0 in list(encode.parse(f.read_bytes()).desc.n_bytes_latent[:7])]
    assert empty, "no committed class-D stream with an empty latent grid left"
    for f in (d_files[0] if d_files[0] != empty[0] else d_files[1], empty[0]):
        out.append((f.name[:12], f.read_bytes(), (240, 416)))
    out.append(("wide32", _generate(WIDE[0], WIDE[1], 15, plants=_wide_plants(PAIRS32, 151)), WIDE))
    assert len(out) == N16 + 1
    return out


@pytest.fixture(scope="module")
def latents(streams, gpu, ccmi_lib):
    from ccmi import decode
    return [decode.decode_latents(b) for _, b, _ in streams]


@pytest.fixture(scope="module")
def planes(streams, gpu, ccmi_lib):
    """{(bitdepth, chroma): [planes per stream]} from decode_batch."""
    from ccmi import decode
    data = [b for _, b, _ in streams]
    ref = {}
    for bitdepth, chroma in ((8, 420), (8, 444), (10, 420), (10, 444)):
        outs = decode.decode_batch(data, output_bitdepth=bitdepth, output_chroma_format=chroma, as_yuv=True)
        ref[(bitdepth, chroma)] = [_planes(o, h, w, bitdepth, chroma) for o, (_, _, (h, w)) in zip(outs, streams)]
    return ref


@pytest.fixture(scope="module")
def source(streams, gpu, ccmi_lib):
    import torch
    from ccmi import decode
    st = decode.LatentStore([b for _, b, _ in streams[:N16]], dtype=torch.int16)
    yield st
    st.close()


@pytest.fixture(scope="module")
def compacted(source, gpu, ccmi_lib):
    st = source.compact()
    yield st
    st.close()


def _net_ints(stream):
    """(upsampling integers, synthesis integers) a store keeps of this stream: counts."""
    from ccmi import encode
    fr = encode.parse(stream)
    d = fr.desc
    blend = d.n_branches if d.n_branches > 1 else 0
    return d.n_ups * d.ups_k + d.n_pre * d.pre_k, fr.nn["syn_w"].size + fr.nn["syn_b"].size - blend


def _reference_images(data, lats, src_store, src_each):
    """Per stream (bytes, mask of the defined bytes): the networks' integers as the source store
    holds them, the grids from the reference."""
    from ccmi import encode
    src = _np(src_store)
    out, pos = [], 0
    for b, lat, nb in zip(data, lats, src_each):
        n_ups, n_syn = _net_ints(b)
        ups = src[pos: pos + 4 * n_ups].view(np.int32)
        at = pos + R.align(4 * n_ups, 16)
        syn = src[at: at + 4 * n_syn].view(np.int32)
        fr = encode.parse(b)
        coded = list(fr.desc.n_bytes_latent[: fr.desc.n_grids])
        grids = [R.pack_grid(np.asarray(v).reshape(h, w)) if nbytes > 0 else None
                 for v, (h, w), nbytes in zip(lat, fr.grid_sizes, coded)]
        out.append(R.stream_image(ups, syn, grids) + (grids,))
        pos += nb
    return out


def _check_image(store, each, refs, what):
    got = _np(store)
    assert sum(each) <= got.size
    pos = 0
    for i, (nb, (img, mask, _)) in enumerate(zip(each, refs)):
        assert nb == len(img), (what, "stream %d: %d bytes, the reference has %d" % (i, nb, len(img)))
        part = got[pos: pos + nb]
        want = np.frombuffer(img, dtype=np.uint8)
        bad = np.flatnonzero((part != want) & mask)
        assert bad.size == 0, (what, "stream %d: %d bytes differ, the first at %d" % (i, bad.size, int(bad[0])))
        pos += nb


def _c_compact(h_src, short=0):
    """ccmi_latents_compact_plan / _measure / compact themselves: store and workspace pre-filled
    with 0xA5, 256 guard bytes behind the store.  -> (rc, handle, store, exact bytes, each)."""
    import torch
    from ccmi import decode
    L = decode._bind_latents()
    n = L.ccmi_latents_count(h_src)
    bound, nws, exact = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    each = (C.c_size_t * n)()
    decode.check(L.ccmi_latents_compact_plan(h_src, C.byref(bound), C.byref(nws)))
    ws = torch.full((max(nws.value, 256),), 0xA5, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    decode.check(L.ccmi_latents_compact_measure(h_src, ws.data_ptr(), ws.numel(), s, C.byref(exact), each))
    assert sum(each) == exact.value <= bound.value and all(e % 256 == 0 and e > 0 for e in each)
    # the measure allocates its own workspace too
    again = C.c_size_t(0)
    decode.check(L.ccmi_latents_compact_measure(h_src, None, 0, s, C.byref(again), None))
    assert again.value == exact.value
    store = torch.full((exact.value + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    ws.fill_(0xA5)
    h = C.c_void_p(None)
    rc = L.ccmi_latents_compact(h_src, store.data_ptr(), exact.value - short, ws.data_ptr(), ws.numel(), s, C.byref(h))
    torch.cuda.synchronize()
    return rc, h, store, exact.value, list(each)


def test_store_bytes_are_the_reference_from_every_source_type(streams, latents, gpu, ccmi_lib):
    """Descriptor tables and payloads against tests/latent_seg_ref.py from an I32 source of every
    stream and I16 / I8 sources of the streams that fit; measure == compact == reference sizes;
    the guard bytes stay; a store one byte short is refused with the fill untouched; the values
    read back are decode_latents'."""
    import ccmi
    import torch
    from ccmi import decode, encode
    L = decode._bind_latents()
    fits8 = [all(-128 <= int(np.min(v)) and int(np.max(v)) <= 127 for v in lat) for lat in latents]
    fits16 = [all(-32768 <= int(np.min(v)) and int(np.max(v)) <= 32767 for v in lat) for lat in latents]
    assert fits8 == [True, True, True, False, True, True, False] and fits16 == [True] * N16 + [False]
    codes = set()
    for ltype in (I8, I16, I32):
        keep = [i for i in range(len(streams)) if ltype == I32 or (fits8[i] if ltype == I8 else fits16[i])]
        data = [streams[i][1] for i in keep]
        lats = [latents[i] for i in keep]
        rc, h_src, src_store, src_bytes, _ = _c_build(data, ltype)
        assert rc == 0 and h_src.value, ccmi.last_error()
        try:
            src_each = []
            for i in range(len(data)):
                t, nb = C.c_int(-1), C.c_size_t(0)
                decode.check(L.ccmi_latents_stream_info(h_src, i, C.byref(t), C.byref(nb)))
                assert t.value == ltype
                src_each.append(nb.value)
            assert sum(src_each) == src_bytes
            refs = _reference_images(data, lats, src_store, src_each)
            before = _np(src_store).copy()
            rc, h, store, nbytes, each = _c_compact(h_src)
            assert rc == 0 and h.value, ccmi.last_error()
            try:
                assert (_np(store[nbytes:]) == 0xA5).all(), "the 256 guard bytes after store_bytes were written"
                assert np.array_equal(_np(src_store), before), "the source store was written"
                _check_image(store, each, refs, "from type %d" % ltype)
                print(f"type {ltype}: {len(data)} streams, source {src_bytes} bytes, compact {nbytes} bytes")
                for i in range(len(data)):
                    t, nb = C.c_int(-1), C.c_size_t(0)
                    decode.check(L.ccmi_latents_stream_info(h, i, C.byref(t), C.byref(nb)))
                    assert (t.value, nb.value) == (SEG, each[i])
                # the new handle does not refer to the source: free it and overwrite its store first
                L.ccmi_latents_free(h_src)
                h_src = C.c_void_p(None)
                src_store.fill_(0x5A)
                for i, (b, lat) in enumerate(zip(data, lats)):
                    got = _c_values(h, i, encode.parse(b).grid_sizes)
                    for l, (g, w) in enumerate(zip(got, lat)):
                        assert np.array_equal(g, np.asarray(w).reshape(-1)), (ltype, i, l)
                # a compact store is no source of a compaction
                a, b2 = C.c_size_t(0), C.c_size_t(0)
                assert L.ccmi_latents_compact_plan(h, C.byref(a), C.byref(b2)) == ccmi.ERR_ARG
                assert "CCMI_LATENT_SEG" in ccmi.last_error()
                assert L.ccmi_latents_compact_measure(h, None, 0, None, C.byref(a), None) == ccmi.ERR_ARG
            finally:
                L.ccmi_latents_free(h)
            for _, _, grids in refs:
                codes |= {int(d) & 7 for g in grids if g is not None for d in g[0]}
        finally:
            L.ccmi_latents_free(h_src)
    assert codes == {0, 1, 2, 3, 4, 5}, codes
    # one byte short: CCMI_ERR_ARG naming the size, nothing written, no handle
    rc, h_src, src_store, _, _ = _c_build([streams[3][1], streams[0][1]], I32)
    assert rc == 0
    try:
        rc, h, store, nbytes, each = _c_compact(h_src, short=1)
        assert rc == ccmi.ERR_ARG and not h.value and str(nbytes) in ccmi.last_error(), ccmi.last_error()
        assert (_np(store) == 0xA5).all(), "a refused compaction wrote to the store"
        # plan-only and resident parts do not mix
        keep, sp, ln = decode._marshal([streams[0][1]])
        hp = C.c_void_p(None)
        decode.check(L.ccmi_latents_decode(sp, ln, 1, I16, None, 0, None, 0, None, C.byref(hp)))
        parts, out = (C.c_void_p * 2)(h_src, hp), C.c_void_p(None)
        assert L.ccmi_latents_concat(parts, 2, C.byref(out)) == ccmi.ERR_ARG and not out.value
        assert "plan-only" in ccmi.last_error()
        L.ccmi_latents_free(hp)
    finally:
        L.ccmi_latents_free(h_src)


def test_python_store_facts(streams, source, compacted, gpu, ccmi_lib):
    import torch
    n = N16
    assert len(compacted) == n and compacted.dtype == "seg" and compacted.stream_dtypes == ["seg"] * n
    assert source.dtype == torch.int16 and source.stream_dtypes == [torch.int16] * n
    assert compacted.nbytes == sum(compacted.stream_nbytes) and source.nbytes == sum(source.stream_nbytes)
    assert all(a <= b for a, b in zip(compacted.stream_nbytes, source.stream_nbytes))
    assert compacted.geometry == source.geometry
    for kw in ({}, {"index": [3, 0, 5], "roi": [(2, 2, 100, 20), None, (64, 32, 200, 100)]}):
        assert compacted.render_geometry(**kw) == source.render_geometry(**kw)  # plans do not depend on the type
    print("bytes per stream, int16 -> seg:", list(zip([s[0] for s in streams], source.stream_nbytes, compacted.stream_nbytes)))


@pytest.mark.parametrize("bitdepth,chroma", [(8, 420), (8, 444), (10, 420), (10, 444)])
def test_whole_frames_are_decode_batch(bitdepth, chroma, streams, planes, compacted, gpu, ccmi_lib):
    kw = dict(output_bitdepth=bitdepth, output_chroma_format=chroma)
    outs = compacted.render(workspace=_filled_ws(compacted, 0xA5, **kw), **kw)
    assert len(outs) == N16
    for i, (o, (name, _, (h, w))) in enumerate(zip(outs, streams)):
        _same(o, planes[(bitdepth, chroma)][i], (0, 0, w, h), chroma, name)


def test_latents_are_decode_latents(streams, latents, compacted, gpu, ccmi_lib):
    for i in range(N16):
        for l, (g, w) in enumerate(zip(compacted.latents(i), latents[i])):
            assert np.array_equal(_np(g).reshape(-1), np.asarray(w).reshape(-1)), (i, l)


def _wide_rects():
    h, w = WIDE
    xs = [0, 63, 64, 65, 127, 128, w]
    rects = [(x0, (3 * k) % 10, x1 - x0, h - (3 * k) % 10 - k % 4)
             for k, (x0, x1) in enumerate((a, b) for a in xs for b in xs if a < b)]
    rects += [(x, 0, 1, h) for x in (63, 64, 65, 127, 128, 149)] + [(0, y, w, 1) for y in (0, 11, 23)]
    rects += [(63, 5, 1, 1), (128, 23, 1, 1)]
    return rects


@pytest.mark.parametrize("chroma", [444, 420])
def test_wide_stream_regions_with_both_workspace_fills(chroma, planes, compacted, gpu, ccmi_lib):
    """Rectangles whose left and right edges sit on columns 63, 64, 65, 127, 128 of the 150-wide
    stream, 1-pixel-wide and 1-pixel-high ones; the workspace pre-filled with 0xA5, then 0x5A."""
    h, w = WIDE
    rects = _wide_rects()
    if chroma == 420:
        rects = [(x & ~1, y & ~1, min(max(rw, 2), w - (x & ~1)), min(max(rh, 2), h - (y & ~1))) for x, y, rw, rh in rects]
    ref = planes[(8, chroma)][3]
    kw = dict(index=[3] * len(rects), roi=rects, output_bitdepth=8, output_chroma_format=chroma)
    assert all(p["windowed"] for p in compacted.roi_plan(kw["index"], rects, 8, chroma))
    for fill in (0xA5, 0x5A):
        outs = compacted.render(workspace=_filled_ws(compacted, fill, **kw), **kw)
        for r, o in zip(rects, outs):
            _same(o, ref, r, chroma, "fill %#x" % fill)


def test_regions_of_the_other_streams(streams, planes, compacted, gpu, ccmi_lib):
    """The small streams (one on the per-frame tail), class D with the empty grid."""
    index = [0, 1, 2, 4, 5, 5, 2]
    rects = [(3, 5, 9, 7), (17, 9, 40, 22), (10, 2, 20, 19), (64, 32, 200, 100), (64, 32, 200, 100), (350, 0, 66, 240),
             (34, 18, 1, 1)]
    for chroma in (444, 420):
        rr = rects if chroma == 444 else [(x & ~1, y & ~1, max(a & ~1, 2), max(b & ~1, 2)) for x, y, a, b in rects]
        kw = dict(index=index, roi=rr, output_bitdepth=8, output_chroma_format=chroma)
        for fill in (0xA5, 0x5A):
            outs = compacted.render(workspace=_filled_ws(compacted, fill, **kw), **kw)
            for j, (i, r, o) in enumerate(zip(index, rr, outs)):
                _same(o, planes[(8, chroma)][i], r, chroma, "frame %d, fill %#x" % (j, fill))


def test_render_model_equals_the_int16_stores(streams, source, compacted, gpu, ccmi_lib):
    import torch
    index = [3, 0, 4, 5, 3, 1]
    rects = [(60, 2, 70, 20), (0, 0, 36, 20), (64, 32, 200, 100), (0, 0, 416, 240), (126, 0, 24, 24), (2, 2, 40, 30)]
    mirror = [0, 1, 0, 1, 1, 0]
    kw = dict(index=index, roi=rects, size=(16, 16), dtype=torch.bfloat16, mirror=mirror)
    a = source.render_model(**kw)
    b = compacted.render_model(**kw)
    assert a.dtype == torch.bfloat16 and tuple(a.shape) == (6, 3, 16, 16)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert source.render_model_workspace_bytes(index, rects, (16, 16)) == compacted.render_model_workspace_bytes(index, rects, (16, 16))


def test_concat_of_three_storage_types(streams, planes, gpu, ccmi_lib):
    """[an int16 store of A, a compacted store of B, an int8 store of C], the parts closed first:
    per-stream reference crops for an index with repeats across all parts, and the tail groups
    of one int16 store of A + B + C built in one call."""
    import torch
    from ccmi import decode
    ia, ib, ic = [0, 2], [3, 4, 5], [1]
    data = [b for _, b, _ in streams[:N16]]
    a = decode.LatentStore([data[i] for i in ia], dtype=torch.int16)
    b16 = decode.LatentStore([data[i] for i in ib], dtype=torch.int16)
    b = b16.compact()
    b16.close()
    c = decode.LatentStore([data[i] for i in ic], dtype=torch.int8)
    cat = decode.LatentStore.concat([a, b, c])
    want_bytes = a.stream_nbytes + b.stream_nbytes + c.stream_nbytes
    for part in (a, b, c):
        part.close()
    order = ia + ib + ic  # stream k of cat is streams[order[k]]
    assert len(cat) == 6 and cat.dtype == "mixed"
    assert cat.stream_dtypes == [torch.int16] * 2 + ["seg"] * 3 + [torch.int8]
    assert cat.stream_nbytes == want_bytes and cat.nbytes == sum(want_bytes)
    one = decode.LatentStore([data[i] for i in order], dtype=torch.int16)
    index = [5, 2, 0, 3, 2, 4, 1, 5, 0, 3, 2]
    sizes = [streams[order[k]][2] for k in index]
    rects = [(2 * (j % 5), 2 * (j % 3), min(w - 8, 40 + 10 * j) & ~1, min(h - 4, 12 + 2 * j) & ~1)
             for j, (h, w) in enumerate(sizes)]
    try:
        for chroma in (444, 420):
            kw = dict(index=index, roi=rects, output_bitdepth=8, output_chroma_format=chroma)
            assert cat.render_geometry(**kw) == one.render_geometry(**kw)
            for fill in (0xA5, 0x5A):
                outs = cat.render(workspace=_filled_ws(cat, fill, **kw), **kw)
                groups = decode.last_tail_groups()
                for j, (k, r, o) in enumerate(zip(index, rects, outs)):
                    _same(o, planes[(8, chroma)][order[k]], r, chroma, "frame %d, fill %#x" % (j, fill))
            one.render(**kw)
            assert decode.last_tail_groups() == groups and groups[0] >= 1
        whole = cat.render(output_chroma_format=444)
        for k, o in enumerate(whole):
            h, w = streams[order[k]][2]
            _same(o, planes[(8, 444)][order[k]], (0, 0, w, h), 444, "whole %d" % k)
        for k in (1, 2, 5):
            want = decode.decode_latents(data[order[k]])
            for g, v in zip(cat.latents(k), want):
                assert np.array_equal(_np(g).reshape(-1), np.asarray(v).reshape(-1)), k
        # a compaction of the int16 / int8 streams of a mixed handle is refused as a whole: it holds SEG streams
        with pytest.raises(decode.CcmiError):
            cat.compact()
    finally:
        cat.close()
        one.close()


def test_int32_wide_stream_renders_from_its_compaction(streams, planes, gpu, ccmi_lib):
    """The 24 x 150 stream with the -32769 / 32768 boundaries: int32 store -> compaction (the
    source closed), whole frame and the column-edge rectangles."""
    import torch
    from ccmi import decode
    st = decode.LatentStore([streams[N16][1]], dtype=torch.int32)
    cp = st.compact()
    st.close()
    assert cp.stream_nbytes[0] < st.stream_nbytes[0]
    rects = [(0, 0, WIDE[1], WIDE[0])] + _wide_rects()[::3]
    kw = dict(index=[0] * len(rects), roi=rects, output_bitdepth=8, output_chroma_format=444)
    for fill in (0xA5, 0x5A):
        outs = cp.render(workspace=_filled_ws(cp, fill, **kw), **kw)
        for r, o in zip(rects, outs):
            _same(o, planes[(8, 444)][N16], r, 444, "fill %#x" % fill)
    cp.close()


def test_q32_stream_compacts_to_codes_16_and_32(gpu, ccmi_lib):
    """d16h0_q32 carries one -40000 and 20000s: int32 everywhere in an element-typed store, one
    32-bit segment here; the whole-frame md5 from the compaction is the pinned one."""
    import torch
    from ccmi import decode
    name = "d16h0_q32"
    data = (S.SYNTH / f"{name}.cool").read_bytes()
    pinned = json.loads((GOLDEN / "synth_md5.json").read_text())["streams"]
    lat = decode.decode_latents(data)
    assert min(int(np.min(v)) for v in lat) == -40000 and max(int(np.max(v)) for v in lat) == 20000
    st = decode.LatentStore([data], dtype=torch.int32)
    cp = st.compact()
    refs = _reference_images([data], [lat], st._store, st.stream_nbytes)
    _check_image(cp._store, cp.stream_nbytes, refs, name)
    codes = [int(d) & 7 for g in refs[0][2] if g is not None for d in g[0]]
    assert 4 in codes and codes.count(5) == 1, sorted(set(codes))  # the one -40000 costs one 32-bit segment
    st.close()
    o, = cp.render(workspace=_filled_ws(cp, 0xA5))
    assert hashlib.md5(b"".join(_np(o[k]).tobytes() for k in "yuv")).hexdigest() == pinned[name]["md5"]
    print(f"{name}: int32 store {st.nbytes} bytes, compact {cp.nbytes} bytes")
    cp.close()
