"""Region decode (ccmi_decode_batch_dev_roi / decode.decode_batch_tensors(roi=...)): the
result is, sample for sample, the crop of the whole-frame decode.  The reference is always code
that existed before the region path: the bytes of decode.decode_batch (themselves pinned to the
reference decoder's md5s and, for the generated streams, shown here to be the C oracle's),
cropped in numpy -- never the region path itself and never whole-frame decode_batch_tensors.

Every call hands the library a workspace filled with 0xA5, so a read of a latent row the ARM
decode skipped, or of a window sample nothing wrote, shows as a mismatch instead of passing
on the data of an earlier whole-frame decode.

Streams with a fused synthesis decode on windows (dec_ups_level_win_batch,
dec_syn_fused_win_batch); the generated stream whose third synthesis layer is 1x1 takes the
per-frame tail on the whole frame and the cropping output kernel (dec_output_tensor_crop)."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import synth_streams as S

GOLDEN = Path(__file__).resolve().parent / "golden"
MD5 = json.loads((GOLDEN / "ref_md5.json").read_text())
FILES = sorted((GOLDEN / "cool").glob("*.cool"))
CLIC = sorted((GOLDEN / "cool" / "clic").glob("*.cool"))
SMALL = ((21, 37), (34, 66), (21, 37))  # the last one with the generic synthesis

pytestmark = pytest.mark.gpu


class Rect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


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
    """The region of a whole-frame decode, as the header defines it."""
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


def _roi_tensors(streams, rects, bitdepth=0, chroma=0, **kw):
    """decode_batch_tensors(roi=...) with a caller workspace filled with 0xA5."""
    import torch
    from ccmi import decode
    _, need = decode.decode_batch_geometry(streams, bitdepth, chroma, roi=rects)
    ws = torch.full((max(need, 256),), 0xA5, dtype=torch.uint8, device="cuda")
    return decode.decode_batch_tensors(streams, bitdepth, chroma, workspace=ws, roi=rects, **kw)


@pytest.fixture(scope="module")
def small(gpu, ccmi_lib):
    """Generated streams (tests/test_decode_tensor_gpu.py's recipe): (21, 37), (34, 66) and
    (21, 37) with a generic synthesis.  The coarse grids are 1 to 5 samples wide."""
    import torch
    from ccmi import encode

    def build(h, w, seed, generic=False):
        fr = encode.parse(S.BASE.read_bytes())
        d = fr.desc
        d.h, d.w = h, w
        if generic:
            # layer 2 (3 -> 3, 3x3, after the fused 1x1 pair) keeps its centre taps only
            c_in, p, parts = d.n_grids, 0, []
            assert d.n_syn_layers >= 3 and d.syn_ks[2] == 3 and d.n_branches == 1
            for l in range(d.n_syn_layers):
                n = d.syn_out[l] * c_in * d.syn_ks[l] ** 2
                wl = fr.nn["syn_w"][p: p + n]
                if l == 2:
                    wl = wl.reshape(d.syn_out[l], c_in, 3, 3)[:, :, 1, 1].reshape(-1)
                parts.append(wl)
                p, c_in = p + n, d.syn_out[l]
            assert p == fr.nn["syn_w"].size
            fr.nn["syn_w"] = np.concatenate(parts)
            d.syn_ks[2] = 1
        g = torch.Generator().manual_seed(seed)
        lat = [torch.round(2.0 * torch.randn(hh * ww, generator=g)).to(torch.int32) for hh, ww in fr.grid_sizes]
        d.ac_max_val_latent = min(65535, max(int(a.abs().max()) for a in lat) + 2)
        return encode.encode_frame(fr, torch.cat(lat).to(gpu), search_counts=True)

    return [build(21, 37, 7), build(34, 66, 9), build(21, 37, 11, generic=True)]


@pytest.fixture(scope="module")
def small_ref(small, gpu, ccmi_lib, oracle_c, tmp_path_factory):
    """{(bitdepth, chroma): [planes of every generated stream]} from decode_batch, whose bytes
    are first shown to be the C oracle's."""
    from ccmi import decode
    tmp = tmp_path_factory.mktemp("roi_small")
    ref = {}
    for bitdepth, chroma in ((8, 420), (8, 444), (10, 420), (10, 444)):
        outs = decode.decode_batch(small, output_bitdepth=bitdepth, output_chroma_format=chroma, as_yuv=True)
        for i, (d, r) in enumerate(zip(small, outs)):
            (tmp / "s.cool").write_bytes(d)
            assert oracle_c.cco_decode_file(str(tmp / "s.cool").encode(), str(tmp / "o.yuv").encode(), bitdepth,
                                            chroma, 0) == 0
            assert (tmp / "o.yuv").read_bytes() == r, f"decode_batch differs from the oracle on generated stream {i}"
        ref[(bitdepth, chroma)] = [_planes(r, h, w, bitdepth, chroma) for r, (h, w) in zip(outs, SMALL)]
    return ref


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
def test_small_frames_every_rect_is_the_crop(idx, chroma, small, small_ref, gpu, ccmi_lib):
    """Corners, strips, the whole frame and 24 seeded rects of each generated frame, all in one
    call (the stream repeated) and three of them alone."""
    from ccmi import decode
    h, w = SMALL[idx]
    planes = small_ref[(8, chroma)][idx]
    rects = _small_rects(h, w, chroma, 100 + idx)
    plan = decode.roi_plan([small[idx]] * len(rects), rects, 8, chroma)
    assert all(p["windowed"] == (idx != 2) for p in plan)
    outs = _roi_tensors([small[idx]] * len(rects), rects, 8, chroma)
    for r, o in zip(rects, outs):
        _same(o, planes, r, chroma, "in one call")
    for r in (rects[4], rects[7], rects[20]):
        o, = _roi_tensors([small[idx]], [r], 8, chroma)
        _same(o, planes, r, chroma, "alone")


@pytest.fixture(scope="module")
def synth(gpu, ccmi_lib):
    """The 10 committed synthetic 416 x 240 streams and their whole-frame planes at 420 / 444,
    from decode_batch (420: the md5s of tests/golden/synth_md5.json, pinned to the reference)."""
    from ccmi import decode
    names = sorted(S.CASES)
    data = [(S.SYNTH / f"{n}.cool").read_bytes() for n in names]
    pinned = json.loads((GOLDEN / "synth_md5.json").read_text())["streams"]
    ref = {}
    for chroma in (420, 444):
        outs = decode.decode_batch(data, output_chroma_format=chroma, as_yuv=True)
        ref[chroma] = [_planes(o, 240, 416, 8, chroma) for o in outs]
        if chroma == 420:
            for n, o in zip(names, outs):
                assert hashlib.md5(o).hexdigest() == pinned[n]["md5"], n
    return names, data, ref


@pytest.mark.parametrize("rect,chroma", [((62, 14, 68, 36), 420), ((63, 15, 65, 33), 444), ((0, 0, 416, 8), 420),
                                         ((0, 200, 416, 40), 420), ((352, 224, 64, 16), 420),
                                         ((0, 140, 416, 40), 420)])
def test_tiles_borders_and_arm_row_bound_at_416x240(rect, chroma, synth, gpu, ccmi_lib):
    """Regions that cross the 64 x 16 pyramid tiles and the synthesis tiles, with odd origin and
    sizes, at the frame's edges; chain, spec and one-latent ARM kernels; block maps -16, 8, 0.
    The q32 cases carry large latents at grid-0 rows 100 and 150: a region whose ARM decode
    stops above them never sees them (no Q32 / BIG flag), one that reaches row 150 reports the
    case's expected bits -- the row bound took effect in all three kernels."""
    from ccmi import decode
    names, data, ref = synth
    plan = decode.roi_plan(data, rect, 0, chroma)
    outs = _roi_tensors(data, rect, 0, chroma)
    flags = decode.last_arm_flags()
    assert len(flags) == len(names)
    for n, o, planes in zip(names, outs, ref[chroma]):
        _same(o, planes, rect, chroma, n)
    rows0 = [p["arm_rows"][0] for p in plan]
    if rect == (0, 200, 416, 40):
        assert all(p["arm_rows"] == [240, 120, 60, 30, 15, 8, 4] for p in plan)
    if rect == (0, 0, 416, 8):
        assert max(rows0) < 100
        for n, f in zip(names, flags):
            wide = S.Q32 if S.kernel_of(n) == "chain" else S.BIG
            assert not f & wide, (n, S.kernel_of(n), f)
    if rect == (0, 140, 416, 40):
        assert 150 < min(rows0) < 240
        for n, f in zip(names, flags):
            assert f == S.CASES[n][5], (n, S.kernel_of(n), f)


def _key(f):
    return "jvet/" + f.name


def test_batch_of_mixed_frame_sizes_stacks_equal_crops(small, small_ref, gpu, ccmi_lib):
    """66 streams in one call (both chunks of dec_host.cpp): the class-D streams twice, a 720p
    class-E stream and the generated (34, 66) stream, one region size of 48 x 32 at seeded even
    origins, stacked.  Frames of three sizes share the region's launches."""
    import torch
    from ccmi import decode
    d_files = [f for f in FILES if f.name.startswith("D-")]
    e_file = [f for f in FILES if f.name.startswith("E-")][3]
    assert len(d_files) == 20
    items = [("c", f) for f in d_files] * 2 + [("c", e_file)] * 12
    for k in range(14):
        items.insert(k * 4 + 3, ("g", 1))
    assert len(items) == 66
    blobs = {f: f.read_bytes() for f in d_files + [e_file]}
    size = {f: (MD5[_key(f)]["h"], MD5[_key(f)]["w"]) for f in blobs}
    rng = np.random.default_rng(5)
    streams, rects = [], []
    for t, x in items:
        h, w = size[x] if t == "c" else SMALL[1]
        streams.append(blobs[x] if t == "c" else small[x])
        rects.append((2 * int(rng.integers(0, (w - 48) // 2 + 1)), 2 * int(rng.integers(0, (h - 32) // 2 + 1)), 48, 32))
    o420 = _roi_tensors(streams, rects, 0, 420, stack=True)
    t420 = decode.last_timing()
    o444 = _roi_tensors(streams, rects, 0, 444, stack=True)
    assert tuple(o420["y"].shape) == (66, 32, 48) and tuple(o420["u"].shape) == tuple(o420["v"].shape) == (66, 16, 24)
    assert tuple(o444.shape) == (66, 3, 32, 48) and o444.dtype == torch.uint8
    assert t420["download"] == 0 and t420["arm_cabac"] > 0 and t420["ups_syn_out"] > 0
    # afterwards: the byte path still has the pinned md5s, and its bytes are the reference
    files = list(blobs)
    ref = {}
    for chroma in (420, 444):
        outs = decode.decode_batch([blobs[f] for f in files], output_chroma_format=chroma, as_yuv=True)
        if chroma == 420:
            assert decode.last_timing()["download"] > 0
            for f, o in zip(files, outs):
                assert hashlib.md5(o).hexdigest() == MD5[_key(f)]["md5"], f.name
        ref[chroma] = {f: _planes(o, size[f][0], size[f][1], 8, chroma) for f, o in zip(files, outs)}
    y, u, v, rgb = _np(o420["y"]), _np(o420["u"]), _np(o420["v"]), _np(o444)
    for i, ((t, x), r) in enumerate(zip(items, rects)):
        p420 = ref[420][x] if t == "c" else small_ref[(8, 420)][x]
        p444 = ref[444][x] if t == "c" else small_ref[(8, 444)][x]
        for g, want in zip((y[i], u[i], v[i]), _crop(p420, r, 420)):
            assert np.array_equal(g, want), (i, t, r)
        for g, want in zip(rgb[i], _crop(p444, r, 444)):
            assert np.array_equal(g, want), (i, t, r)


def _c_roi(streams, rects, sample, bitdepth, chroma, gpu, cap_short=0, ws_div=1):
    """ccmi_decode_batch_dev_roi itself: frame i at i samples past a 16-byte boundary inside a
    buffer filled with 0xA5, the workspace filled with 0xA5 too.  -> (rc, host bytes, offsets,
    sample counts, slot size)."""
    import torch
    from ccmi import decode
    n = len(streams)
    L = decode._bind_dev()
    keep = [C.create_string_buffer(s, len(s)) for s in streams]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in keep])
    ln = (C.c_size_t * n)(*[len(s) for s in streams])
    arr = (Rect * n)(*[Rect(*r) for r in rects])
    ssize = (1, 2, 4)[sample]
    elems = [w * h + 2 * (h // 2) * (w // 2) if chroma == 420 else 3 * w * h for x, y, w, h in rects]
    slot = (max(elems) * ssize + 64 + 15) // 16 * 16 + 16
    buf = torch.full((n * slot,), 0xA5, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    offs = [i * slot + 32 + (i % 4) * ssize for i in range(n)]
    op = (C.c_void_p * n)(*[buf.data_ptr() + o for o in offs])
    cap = (C.c_size_t * n)(*[e * ssize - cap_short * ssize for e in elems])
    geom, need = (decode.FrameGeom * n)(), C.c_size_t(0)
    # the plan is made for the valid twin of a failing call (same streams, in-frame rects)
    rc = L.ccmi_decode_batch_dev_roi_plan(sp, ln, n, arr, bitdepth, chroma, sample, geom, None, C.byref(need))
    nws = max(need.value, 256) if rc == 0 else 1 << 20
    ws = torch.full((nws,), 0xA5, dtype=torch.uint8, device=gpu)
    rc = L.ccmi_decode_batch_dev_roi(sp, ln, n, arr, op, cap, sample, bitdepth, chroma, ws.data_ptr(), nws // ws_div,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), offs, elems, slot


@pytest.mark.parametrize("sample,chroma", [(0, 420), (1, 420), (2, 420), (1, 444)])
def test_c_abi_samples_alignment_and_no_stray_writes(sample, chroma, small, small_ref, gpu, ccmi_lib):
    """u8 at 8 bits, u16 and f32 at 10: region widths with w mod 4 = 1, 2, 3, output pointers
    0..3 samples past a 16-byte boundary, the window tail (fused stream) and the cropping output
    kernel (generic stream) side by side.  The bytes around each frame keep their fill."""
    from ccmi import decode
    bitdepth = 8 if sample == 0 else 10
    idx = [0, 2, 0, 2, 0, 2, 1, 1]
    rects = [(2, 4, 5, 9), (2, 4, 5, 9), (6, 2, 6, 7), (6, 2, 6, 7), (10, 0, 7, 21), (10, 0, 7, 21), (0, 0, 66, 3),
             (18, 20, 47, 14)]
    rc, host, offs, elems, slot = _c_roi([small[i] for i in idx], rects, sample, bitdepth, chroma, gpu)
    assert rc == 0, decode.lib().ccmi_last_error()
    ssize = (1, 2, 4)[sample]
    maxv = np.float32((1 << bitdepth) - 1)
    for i, (o, e, r) in enumerate(zip(offs, elems, rects)):
        want = np.concatenate([p.reshape(-1) for p in _crop(small_ref[(bitdepth, chroma)][idx[i]], r, chroma)])
        assert want.size == e
        got = host[o: o + e * ssize]
        if sample == 2:
            assert got.view(np.float32).tobytes() == (want.astype(np.float32) / maxv).tobytes(), (i, r)
        else:
            assert got.tobytes() == want.tobytes(), (i, r)
        lo = offs[i - 1] + elems[i - 1] * ssize if i else 0
        assert (host[lo: o] == 0xA5).all() and (host[o + e * ssize: (i + 1) * slot] == 0xA5).all(), (i, r)


def test_odd_rgb_frame_corners(gpu, ccmi_lib):
    """The committed CLIC stream with odd width and height, RGB 444: the last sample, the
    bottom-right and the top-left 64 x 64, against the PPM bytes of decode_batch."""
    from ccmi import decode, encode
    hit = [f for f in CLIC if encode.parse(f.read_bytes()).desc.h % 2 == 1 and encode.parse(f.read_bytes()).desc.w % 2 == 1]
    assert hit, "no committed CLIC stream with odd width and height left"
    data = hit[0].read_bytes()
    d = encode.parse(data).desc
    H, W = d.h, d.w
    assert (H, W) == (1725, 1145)
    rects = [(W - 1, H - 1, 1, 1), (W - 64, H - 64, 64, 64), (0, 0, 64, 64)]
    outs = _roi_tensors([data] * 3, rects)
    ppm, = decode.decode_batch([data], as_yuv=False)
    hdr = b"P6\n%d %d\n255\n" % (W, H)
    assert ppm.startswith(hdr)
    full = np.frombuffer(ppm[len(hdr):], dtype="u1").reshape(H, W, 3).transpose(2, 0, 1)
    for r, o in zip(rects, outs):
        assert tuple(o.shape) == (3, r[3], r[2])
        _same(o, list(full), r, 444, hit[0].name)


def test_errors_leave_the_output_untouched(small, gpu, ccmi_lib):
    from ccmi import decode
    import ccmi
    ok = [(2, 4, 8, 8), (2, 4, 8, 8)]
    streams = [small[0], small[2]]
    for what, rects, chroma, kw in (
        ("odd origin at 420", [(2, 4, 8, 8), (3, 4, 8, 8)], 420, {}),
        ("rect leaving the frame", [(2, 4, 8, 8), (30, 4, 8, 8)], 444, {}),
        ("out_caps short by one sample", ok, 420, {"cap_short": 1}),
        ("half the planned workspace", ok, 420, {"ws_div": 2}),
    ):
        rc, host, offs, elems, slot = _c_roi(streams, rects, 0, 8, chroma, gpu, **kw)
        assert rc == ccmi.ERR_ARG and decode.lib().ccmi_last_error(), what
        assert (host == 0xA5).all(), what
        assert decode.last_arm_flags() == [], what  # a failed call reports no stream
    with pytest.raises(decode.CcmiError):
        decode.decode_batch_tensors(streams, output_chroma_format=420, roi=(3, 4, 8, 8))
    with pytest.raises(decode.CcmiError):
        decode.decode_batch_tensors(streams, roi=[(0, 0, 8, 8), (30, 20, 8, 8)])
    with pytest.raises(ValueError):
        decode.decode_batch_tensors(streams, roi=[(0, 0, 8, 8), (0, 0, 9, 8)], stack=True)
