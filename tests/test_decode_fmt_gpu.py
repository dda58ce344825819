"""Formatted output (ccmi_decode_batch_dev_fmt / ccmi_latents_render_fmt; decode.decode_batch_model
and LatentStore.render_model): three full-size channels, RGB, normalised, float32 / float16 /
bfloat16, any strides, mirror, written by the decoder's output kernel.

The reference is never the new code and never decode_batch_tensors: the bytes of
decode.decode_batch at the same bitdepth and chroma (pinned elsewhere to the reference decoder's
md5s and the C oracle), split into planes and cropped in numpy as tests/test_latent_store_gpu.py
does, then the contract of ccmi.h restated with torch CPU float32 operations in the stated
order -- sample / maxv, ((p0 + a p1) + b p2) + o, clamp, * scale, + bias, each its own rounded
float32 operation, then .to(dtype), round to nearest even.  Every constant is rounded to
float32 first (numpy), so no operation sees a double.  The comparison is BITWISE for all three
element types: there is no tolerance, every step is one correctly rounded operation.

The generated streams are the region tests': 21 x 37, 34 x 66 and 21 x 37 with a generic
synthesis (per-frame tail, cropping output kernel)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import synth_streams as S

GOLDEN = Path(__file__).resolve().parent / "golden"
FILES = sorted((GOLDEN / "cool").glob("*.cool"))
SMALL = ((21, 37), (34, 66), (21, 37))  # the last one with the generic synthesis
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# io.yuv2rgb's (a, b, o) for R, G, B
YUV2RGB = ((-0.000007154783816076815, 1.4019975662231445, -179.45477266423404),
           (-0.3441331386566162, -0.7141380310058594, 135.45870971679688),
           (1.7720025777816772, 0.00001542569043522235, -226.8183044444304))

pytestmark = pytest.mark.gpu


def _dtypes():
    import torch
    return (torch.float32, torch.float16, torch.bfloat16)


def _f32(v):
    """the float32 rounding of a Python float, as a Python float"""
    return float(np.float32(v))


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
    assert x % 2 == 0 and y % 2 == 0 and w % 2 == 0 and h % 2 == 0
    return [planes[0][y: y + h, x: x + w]] + [p[y // 2: y // 2 + h // 2, x // 2: x // 2 + w // 2] for p in planes[1:]]


def _want(planes, rect, bitdepth, chroma, yuv, colour="rgb", mean=None, std=None, dtype=None, mirror=False):
    """The contract on the CPU: [3, h, w] of dtype."""
    import torch
    dtype = dtype or torch.float32
    s = [torch.from_numpy(np.ascontiguousarray(p).astype(np.int32)) for p in _crop(planes, rect, chroma)]
    if chroma == 420:  # nearest x2: pixel (y, x) takes the 420 plane's (y >> 1, x >> 1)
        s = [s[0]] + [p.repeat_interleave(2, 0).repeat_interleave(2, 1) for p in s[1:]]
    assert s[1].shape == s[0].shape == s[2].shape
    maxv = float((1 << bitdepth) - 1)
    p = [t.to(torch.float32) / maxv for t in s]
    q = p
    if colour == "rgb" and yuv:
        q = []
        for a, b, o in YUV2RGB:
            a, b, o = _f32(a), _f32(b), _f32(o / 255.0)
            t = ((p[0] + a * p[1]) + b * p[2]) + o
            q.append(t.clamp(0.0, 1.0))
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    r = []
    for c in range(3):
        scale, bias = _f32(1.0 / std[c]), _f32(-mean[c] / std[c])
        r.append(q[c] * scale + bias)
    out = torch.stack(r)
    assert out.dtype == torch.float32
    out = out.to(dtype)
    return out.flip(-1) if mirror else out


def _bits(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        c, y, x = bad[0]
        raise AssertionError((what, "%d of %d elements differ" % (len(bad), g.size), "first at c %d y %d x %d" % (c, y, x),
                              float(got[c, y, x]), float(want[c, y, x])))


def _generate(h, w, seed, generic=False):
    """The region tests' recipe (tests/test_latent_store_gpu.py)."""
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
    d.ac_max_val_latent = min(65535, max(int(a.abs().max()) for a in lat) + 2)
    return encode.encode_frame(fr, torch.cat(lat).cuda(), search_counts=True)


@pytest.fixture(scope="module")
def small(gpu, ccmi_lib):
    from ccmi import decode
    data = [_generate(21, 37, 7), _generate(34, 66, 9), _generate(21, 37, 11, generic=True)]
    plan = decode.roi_plan(data, (0, 0, 8, 8), output_chroma_format=444)
    assert [p["windowed"] for p in plan] == [True, True, False]  # the third takes the per-frame tail
    return data


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
def small_store(small, gpu, ccmi_lib):
    from ccmi import decode
    st = decode.LatentStore(small)
    yield st
    st.close()


@pytest.fixture(scope="module")
def class_d(gpu, ccmi_lib):
    """Two committed class-D 416 x 240 streams (the second one has an empty latent grid) and
    their planes at their own format (8 bits, 420)."""
    from ccmi import decode, encode
    d_files = [f for f in FILES if f.name.startswith("D-")]
    empty = [f for f in d_files if 0 in list(encode.parse(f.read_bytes()).desc.n_bytes_latent[:7])]
    assert empty, "no committed class-D stream with an empty latent grid left"
    files = [d_files[0] if d_files[0] != empty[0] else d_files[1], empty[0]]
    data = [f.read_bytes() for f in files]
    outs = decode.decode_batch(data, as_yuv=True)
    return data, [_planes(o, 240, 416, 8, 420) for o in outs]


def _filled_ws(store, fill, **kw):
    import torch
    _, need = store.render_geometry(dtype=torch.float32, **kw)
    return torch.full((max(need, 256),), fill, dtype=torch.uint8, device="cuda")


def _whole(i):
    h, w = SMALL[i]
    return (0, 0, w, h)


@pytest.mark.parametrize("bitdepth", (8, 10))
def test_whole_frames_444_every_elem_and_colour(small, small_ref, bitdepth):
    """decode_batch_model on the coded streams: the batched whole-frame tail (21 x 37, 34 x 66) and
    the per-frame tail (the generic 21 x 37), every element type x colour, with and without
    mean / std.  The two 21 x 37 frames are stacked: the second starts at an odd element."""
    from ccmi import decode
    planes = small_ref[(bitdepth, 444)]
    for group in ((0, 2), (1,)):
        for dtype in _dtypes():
            for colour in ("rgb", "asis"):
                for mean, std in ((None, None), (MEAN, STD)):
                    got = decode.decode_batch_model([small[i] for i in group], colour=colour, mean=mean, std=std,
                                                    dtype=dtype, output_bitdepth=bitdepth, output_chroma_format=444)
                    assert tuple(got.shape) == (len(group), 3) + SMALL[group[0]] and got.is_contiguous()
                    for j, i in enumerate(group):
                        _same(got[j], _want(planes[i], _whole(i), bitdepth, 444, True, colour, mean, std, dtype),
                              (bitdepth, i, dtype, colour, mean))


@pytest.mark.parametrize("fill", (0xA5, 0x5A))
def test_stacked_odd_frames_half_types(small_store, small_ref, fill):
    """21 x 37 frames back to back in fp16 and bf16: frame 1 starts at element 2331, so every row
    of it has its own lead-in and the partial-group stores run; render workspace pre-filled."""
    import torch
    planes = small_ref[(8, 444)]
    index = [0, 2, 0]
    for dtype in (torch.float16, torch.bfloat16):
        ws = _filled_ws(small_store, fill, index=index, output_chroma_format=444)
        got = small_store.render_model(index=index, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444,
                                       workspace=ws)
        assert got.data_ptr() % 8 == 0 and (got[1].data_ptr() // 2) % 2 == 1
        for j, i in enumerate(index):
            _same(got[j], _want(planes[i], _whole(i), 8, 444, True, "rgb", MEAN, STD, dtype), (dtype, j))


@pytest.mark.parametrize("rect", ((36, 20, 1, 1), (0, 0, 3, 5), (5, 3, 7, 2), (30, 0, 7, 21)))
def test_regions_444(small, small_store, small_ref, rect):
    """Regions of the 21 x 37 frames at 444: the batched window tail and the per-frame cropping
    form, from the coded streams and from the store."""
    from ccmi import decode
    for bitdepth in (8, 10):
        planes = small_ref[(bitdepth, 444)]
        for k, dtype in enumerate(_dtypes()):
            colour = ("rgb", "asis")[(k + bitdepth) % 2]
            got = decode.decode_batch_model([small[0], small[2]], roi=rect, colour=colour, mean=MEAN, std=STD, dtype=dtype,
                                            output_bitdepth=bitdepth, output_chroma_format=444)
            ws = _filled_ws(small_store, 0xA5 if k else 0x5A, index=[0, 2], roi=rect, output_bitdepth=bitdepth,
                            output_chroma_format=444)
            ren = small_store.render_model(index=[0, 2], roi=rect, colour=colour, mean=MEAN, std=STD, dtype=dtype,
                                           output_bitdepth=bitdepth, output_chroma_format=444, workspace=ws)
            for j, i in enumerate((0, 2)):
                want = _want(planes[i], rect, bitdepth, 444, True, colour, MEAN, STD, dtype)
                _same(got[j], want, ("decode", rect, bitdepth, dtype, i))
                _same(ren[j], want, ("render", rect, bitdepth, dtype, i))


@pytest.mark.parametrize("rect", ((0, 0, 2, 2), (64, 32, 2, 2), (2, 4, 6, 10), (10, 0, 56, 34)))
def test_regions_420(small, small_store, small_ref, rect):
    """Regions of the 34 x 66 frame at 420: chroma from the even row and column, upsampled."""
    from ccmi import decode
    for bitdepth in (8, 10):
        planes = small_ref[(bitdepth, 420)][1]
        for k, dtype in enumerate(_dtypes()):
            colour = ("rgb", "asis")[(k + bitdepth // 2) % 2]
            want = _want(planes, rect, bitdepth, 420, True, colour, MEAN, STD, dtype)
            got = decode.decode_batch_model([small[1]], roi=rect, colour=colour, mean=MEAN, std=STD, dtype=dtype,
                                            output_bitdepth=bitdepth, output_chroma_format=420)
            _same(got[0], want, ("decode", rect, bitdepth, dtype))
            ws = _filled_ws(small_store, 0x5A if k else 0xA5, index=[1], roi=rect, output_bitdepth=bitdepth,
                            output_chroma_format=420)
            ren = small_store.render_model(index=[1], roi=rect, colour=colour, mean=MEAN, std=STD, dtype=dtype,
                                           output_bitdepth=bitdepth, output_chroma_format=420, workspace=ws)
            _same(ren[0], want, ("render", rect, bitdepth, dtype))


def test_whole_frames_420(small, small_ref):
    """The streams' own 420 on whole even-sized frames is the 34 x 66 one; the odd 21 x 37 frames
    are refused at 420 (and nothing else): the message suggests 444."""
    import torch
    from ccmi import CcmiError, decode
    got = decode.decode_batch_model([small[1]], dtype=torch.bfloat16, mean=MEAN, std=STD)
    _same(got[0], _want(small_ref[(8, 420)][1], _whole(1), 8, 420, True, "rgb", MEAN, STD, torch.bfloat16), "34 x 66")
    with pytest.raises(CcmiError, match="444"):
        decode.decode_batch_model([small[0]])


def test_class_d_bf16_rgb_normalised(class_d):
    """Two class-D streams (one with an empty latent grid): the whole frame and a 64 x 64 region."""
    import torch
    from ccmi import decode
    data, planes = class_d
    for rect in (None, (352, 176, 64, 64)):
        got = decode.decode_batch_model(data, roi=rect, mean=MEAN, std=STD, dtype=torch.bfloat16)
        r = rect or (0, 0, 416, 240)
        assert tuple(got.shape) == (2, 3, r[3], r[2])
        for j in range(2):
            _same(got[j], _want(planes[j], r, 8, 420, True, "rgb", MEAN, STD, torch.bfloat16), (rect, j))
    with decode_store(data) as st:
        ren = st.render_model(roi=(352, 176, 64, 64), mean=MEAN, std=STD, dtype=torch.bfloat16)
        assert np.array_equal(_bits(ren.reshape(6, 64, 64)), _bits(got.reshape(6, 64, 64)))


class decode_store:
    def __init__(self, data):
        from ccmi import decode
        self.st = decode.LatentStore(data)

    def __enter__(self):
        return self.st

    def __exit__(self, *exc):
        self.st.close()


def test_kodak_rgb_identity():
    """An RGB stream: CCMI_COLOUR_RGB applies no matrix (q = p), so 'rgb' and 'asis' are the same
    tensor; the reference planes come from the PPM bytes."""
    import torch
    from ccmi import decode
    f = [f for f in sorted((GOLDEN / "cool").rglob("kodim*.cool"))][0]
    data = f.read_bytes()
    geom, _ = decode.decode_batch_geometry([data])
    h, w = geom[0]["height"], geom[0]["width"]
    assert geom[0]["frame_data_type"] == 0 and geom[0]["chroma"] == 444
    ppm, = decode.decode_batch([data], as_yuv=False)
    hdr = b"P6\n%d %d\n255\n" % (w, h)
    assert ppm.startswith(hdr)
    planes = list(np.frombuffer(ppm[len(hdr):], dtype="u1").reshape(h, w, 3).transpose(2, 0, 1))
    rect = (w - 200, h - 120, 200, 120)
    for dtype, colour in ((torch.bfloat16, "rgb"), (torch.float32, "asis"), (torch.float16, "rgb")):
        got = decode.decode_batch_model([data], roi=rect, colour=colour, mean=MEAN, std=STD, dtype=dtype)
        _same(got[0], _want(planes, rect, 8, 444, False, colour, MEAN, STD, dtype), (dtype, colour))


@pytest.mark.parametrize("width", (1, 2, 3, 7))
def test_mirror_mixed_flags_444(small_store, small_ref, width):
    import torch
    planes = small_ref[(8, 444)]
    index, flags = [0, 2, 0, 2], [True, False, False, True]
    rect = (37 - width - 4, 3, width, 6)
    for dtype in _dtypes():
        got = small_store.render_model(index=index, roi=rect, mean=MEAN, std=STD, dtype=dtype, mirror=flags,
                                       output_chroma_format=444)
        for j, (i, m) in enumerate(zip(index, flags)):
            _same(got[j], _want(planes[i], rect, 8, 444, True, "rgb", MEAN, STD, dtype, mirror=m), (width, dtype, j, m))
    nhwc = small_store.render_model(index=index, roi=rect, dtype=torch.float16, mirror=flags, channels_last=True,
                                    output_chroma_format=444)
    for j, (i, m) in enumerate(zip(index, flags)):
        _same(nhwc[j], _want(planes[i], rect, 8, 444, True, dtype=torch.float16, mirror=m), ("nhwc", width, j, m))


def test_mirror_width_56_at_420(small, small_store, small_ref):
    from ccmi import decode
    planes = small_ref[(8, 420)][1]
    rect = (10, 0, 56, 34)
    for dtype in _dtypes():
        got = small_store.render_model(index=[1, 1, 1], roi=rect, mean=MEAN, std=STD, dtype=dtype, mirror=[True, False, True])
        dec = decode.decode_batch_model([small[1]] * 2, roi=rect, mean=MEAN, std=STD, dtype=dtype, mirror=[False, True],
                                        channels_last=True)
        for j, m in enumerate((True, False, True)):
            _same(got[j], _want(planes, rect, 8, 420, True, "rgb", MEAN, STD, dtype, mirror=m), (dtype, j, m))
        for j, m in enumerate((False, True)):
            _same(dec[j], _want(planes, rect, 8, 420, True, "rgb", MEAN, STD, dtype, mirror=m), ("nhwc", dtype, j, m))


def test_channels_last(small, small_store, small_ref):
    """An [n, h, w, 3] allocation returned as its [n, 3, h, w] view; odd width and odd row starts."""
    from ccmi import decode
    for dtype in _dtypes():
        got = decode.decode_batch_model([small[0], small[2]], dtype=dtype, channels_last=True, mean=MEAN, std=STD,
                                        output_chroma_format=444)
        assert tuple(got.shape) == (2, 3, 21, 37) and tuple(got.stride()) == (21 * 37 * 3, 1, 37 * 3, 3)
        for j, i in enumerate((0, 2)):
            _same(got[j], _want(small_ref[(8, 444)][i], _whole(i), 8, 444, True, "rgb", MEAN, STD, dtype), (dtype, i))
        ren = small_store.render_model(index=[1], dtype=dtype, channels_last=True, colour="asis")
        assert tuple(ren.stride()) == (34 * 66 * 3, 1, 66 * 3, 3)
        _same(ren[0], _want(small_ref[(8, 420)][1], _whole(1), 8, 420, True, "asis", dtype=dtype), (dtype, "420"))


def _sentinel_canvas(shape, dtype):
    """A tensor whose every element holds a bit pattern no output produces (a NaN payload)."""
    import torch
    if dtype == torch.float32:
        return torch.full(shape, 0x7FC12345, dtype=torch.int32, device="cuda").view(torch.float32), 0x7FC12345
    return torch.full(shape, 0x7FC1, dtype=torch.int16, device="cuda").view(dtype), 0x7FC1


def test_out_views_into_a_canvas(small_store, small_ref):
    """Two 21 x 37 tiles written into a [3, 40, 80] canvas at different offsets: the tiles hold
    the frames, every other element still holds the sentinel."""
    planes = small_ref[(8, 444)]
    for dtype in _dtypes():
        canvas, pat = _sentinel_canvas((3, 40, 80), dtype)
        spots = ((1, 3), (18, 41))
        tiles = [canvas[:, y: y + 21, x: x + 37] for y, x in spots]
        ret = small_store.render_model(index=[0, 2], out=tiles, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        assert ret[0] is tiles[0] and ret[1] is tiles[1]
        mask = np.ones((3, 40, 80), dtype=bool)
        for (y, x), i in zip(spots, (0, 2)):
            _same(canvas[:, y: y + 21, x: x + 37], _want(planes[i], _whole(i), 8, 444, True, "rgb", MEAN, STD, dtype),
                  (dtype, i))
            mask[:, y: y + 21, x: x + 37] = False
        assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), dtype


def test_padded_rows_and_stride_x_2(small, small_ref):
    """stride_y padded and stride_x = 2: the one-store-per-element path; the gaps keep the sentinel."""
    from ccmi import decode
    planes = small_ref[(8, 420)][1]
    rect = (2, 4, 6, 10)
    for dtype in _dtypes():
        base, pat = _sentinel_canvas((2, 3, 10, 17), dtype)
        views = [base[j, :, :, 0:12:2] for j in range(2)]
        assert tuple(views[0].stride()) == (170, 17, 2)
        decode.decode_batch_model([small[1]] * 2, roi=rect, out=views, mirror=[False, True], dtype=dtype)
        mask = np.ones((2, 3, 10, 17), dtype=bool)
        mask[:, :, :, 0:12:2] = False
        for j in range(2):
            _same(views[j], _want(planes, rect, 8, 420, True, dtype=dtype, mirror=bool(j)), (dtype, j))
        assert (_bits(base)[mask] == np.array(pat).astype(_bits(base).dtype)).all(), dtype


def test_decode_and_render_agree(small, small_store):
    """decode_batch_model and LatentStore.render_model, bit for bit, with repeats and per-frame regions."""
    from ccmi import decode
    index = [1, 1, 0]
    rects = [(2, 4, 6, 10), (10, 0, 6, 10), (5, 3, 6, 10)]
    for dtype in _dtypes():
        for kw in (dict(colour="rgb", mean=MEAN, std=STD), dict(colour="asis", channels_last=True, mirror=[1, 0, 1])):
            a = decode.decode_batch_model([small[i] for i in index], roi=rects, dtype=dtype, output_chroma_format=444, **kw)
            ws = _filled_ws(small_store, 0xA5, index=index, roi=rects, output_chroma_format=444)
            b = small_store.render_model(index=index, roi=rects, dtype=dtype, output_chroma_format=444, workspace=ws, **kw)
            assert a.shape == b.shape == (3, 3, 10, 6) and a.stride() == b.stride()
            assert np.array_equal(_bits(a), _bits(b)), (dtype, kw)
            ws = _filled_ws(small_store, 0x5A, index=index, roi=rects, output_chroma_format=444)
            c = small_store.render_model(index=index, roi=rects, dtype=dtype, output_chroma_format=444, workspace=ws, **kw)
            assert np.array_equal(_bits(b), _bits(c)), (dtype, kw)


def test_python_argument_errors(small, small_store):
    import torch
    from ccmi import decode
    with pytest.raises(ValueError, match="one size"):
        decode.decode_batch_model(small, output_chroma_format=444)
    with pytest.raises(ValueError, match="dtype"):
        decode.decode_batch_model(small[:1], dtype=torch.uint8)
    with pytest.raises(ValueError, match="colour"):
        small_store.render_model(index=[0], colour="bgr", output_chroma_format=444)
    with pytest.raises(ValueError, match="mirror"):
        small_store.render_model(index=[0, 2], mirror=[True], output_chroma_format=444)
    good = torch.zeros(3, 21, 37, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        small_store.render_model(index=[0], out=[good[:, :20]], output_chroma_format=444)
    with pytest.raises(ValueError, match="stride"):
        small_store.render_model(index=[0, 2], out=[good, torch.zeros(3, 21, 40, device="cuda")[:, :, :37]],
                                 output_chroma_format=444)


class _Fmt(C.Structure):
    _fields_ = [("elem", C.c_int), ("colour", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3),
                ("stride_c", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("mirror", C.c_void_p)]


def test_errors_leave_the_destination_untouched(small, small_store):
    """Each plan-time error through the GPU entry points (real device pointers and workspace):
    CCMI_ERR_ARG and a sentinel-filled destination that still holds the sentinel."""
    import torch
    import ccmi
    from ccmi import decode
    L = decode._bind_fmt()
    dst = torch.full((2, 4096), 0x5AA5, dtype=torch.int16, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    data = [small[1], small[1]]
    keep, sp, ln = decode._marshal(data)
    stream = torch.cuda.current_stream().cuda_stream

    def fmt(elem=2, colour=1, scale=1.0, strides=(0, 0, 0)):
        f = _Fmt(elem=elem, colour=colour)
        for c in range(3):
            f.scale[c], f.bias[c] = scale, 0.0
        f.stride_c, f.stride_y, f.stride_x = strides
        return f

    def run(f, rects, caps=(8192, 8192), ptrs=None, chroma=0, store=False):
        arr = (decode.Rect * 2)(*[decode.Rect(*r) for r in rects])
        op = (C.c_void_p * 2)(*(ptrs or [dst[0].data_ptr(), dst[1].data_ptr()]))
        cp = (C.c_size_t * 2)(*caps)
        if store:
            idx = (C.c_int * 2)(1, 1)
            return L.ccmi_latents_render_fmt(small_store._handle(), idx, 2, arr, op, cp, C.byref(f), 0, chroma,
                                             ws.data_ptr(), ws.numel(), stream)
        return L.ccmi_decode_batch_dev_fmt(sp, ln, 2, arr, op, cp, C.byref(f), 0, chroma, ws.data_ptr(), ws.numel(), stream)

    ok = [(0, 0, 8, 4), (2, 4, 8, 4)]
    need = (2 * 32 + 3 * 8 + 7 + 1) * 2
    cases = [
        ("element", fmt(elem=3), ok, {}),
        ("colour", fmt(colour=5), ok, {}),
        ("finite", fmt(scale=float("inf")), ok, {}),
        ("finite", fmt(scale=float("nan")), ok, {}),
        ("stride", fmt(strides=(32, -8, 1)), ok, {}),
        ("alias", fmt(strides=(1, 1, 1)), ok, {}),
        ("alias", fmt(strides=(32, 7, 1)), ok, {}),
        ("even", fmt(), [ok[0], (2, 4, 7, 4)], {}),
        ("even", fmt(), [ok[0], (2, 4, 8, 3)], {}),
        ("need %d" % need, fmt(), ok, {"caps": (need, need - 2)}),
        ("aligned", fmt(), ok, {"ptrs": [dst[0].data_ptr(), dst[1].data_ptr() + 1]}),
        ("outside", fmt(), [ok[0], (60, 30, 8, 8)], {}),
    ]
    for word, f, rects, kw in cases:
        for store in (False, True):
            rc = run(f, rects, store=store, **kw)
            assert rc == 1 and word in ccmi.last_error(), (word, store, rc, ccmi.last_error())
            torch.cuda.synchronize()
            assert bool((dst == 0x5AA5).all()), (word, store)
    # the same call with nothing wrong writes both frames
    assert run(fmt(), ok) == 0, ccmi.last_error()
    torch.cuda.synchronize()
    assert bool((dst[:, :96] != 0x5AA5).all()) and bool((dst[:, 96:] == 0x5AA5).all())
