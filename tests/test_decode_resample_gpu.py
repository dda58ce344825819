"""Resampled formatted output (ccmi_decode_batch_dev_rs / ccmi_latents_render_rs;
decode.decode_batch_model(size=...) and LatentStore.render_model(size=...)): every region, of any
size, resampled to one output size by the antialiased triangle filter in the decoder's output
stage, and frames of different region sizes sharing the tail's launches.

The reference is never the new code: the bytes of decode.decode_batch, split into planes and
cropped in numpy, steps 1-3 of the ccmi_tensor_fmt contract restated with torch CPU float32
operations as tests/test_decode_fmt_gpu.py does, steps 3a-3c in numpy float32 one rounded
operation at a time (tests/resample_ref.py, pinned by tests/test_decode_resample_ref.py), then
scale, bias and .to(dtype).  Every comparison is BITWISE for float32, float16 and bfloat16.

The streams are the formatted-output tests': 21 x 37, 34 x 66 and 21 x 37 with a generic
synthesis (per-frame tail), generated; and one committed class-D 416 x 240 stream."""
from pathlib import Path

import numpy as np
import pytest

import resample_ref as R
from test_decode_fmt_gpu import MEAN, SMALL, STD, YUV2RGB, _bits, _crop, _f32, _generate, _planes, _same, _sentinel_canvas

GOLDEN = Path(__file__).resolve().parent / "golden"

pytestmark = pytest.mark.gpu


def _dtypes():
    import torch
    return (torch.float32, torch.float16, torch.bfloat16)


_CACHE = {}


def _resampled(key, planes, rect, size, bitdepth, chroma, colour):
    """Steps 1-3 (torch CPU float32) and 3a-3c (numpy float32): [3, out_h, out_w] float32, computed
    once per (stream, rect, size, format) and shared by the element types and layouts."""
    import torch
    key = (key, rect, size, bitdepth, chroma, colour)
    if key not in _CACHE:
        s = [torch.from_numpy(np.ascontiguousarray(p).astype(np.int32)) for p in _crop(planes, rect, chroma)]
        if chroma == 420:
            s = [s[0]] + [p.repeat_interleave(2, 0).repeat_interleave(2, 1) for p in s[1:]]
        maxv = float((1 << bitdepth) - 1)
        p = [t.to(torch.float32) / maxv for t in s]
        q = p
        if colour == "rgb":
            q = []
            for a, b, o in YUV2RGB:
                a, b, o = _f32(a), _f32(b), _f32(o / 255.0)
                q.append((((p[0] + a * p[1]) + b * p[2]) + o).clamp(0.0, 1.0))
        q = torch.stack(q)
        assert q.dtype == torch.float32
        r = R.resample(q.numpy(), size[0], size[1])
        r.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def _want(key, planes, rect, size, bitdepth=8, chroma=444, colour="rgb", mean=None, std=None, dtype=None, mirror=False):
    import torch
    dtype = dtype or torch.float32
    r = torch.from_numpy(_resampled(key, planes, rect, size, bitdepth, chroma, colour).copy())
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    out = torch.stack([r[c] * _f32(1.0 / std[c]) + _f32(-mean[c] / std[c]) for c in range(3)])
    assert out.dtype == torch.float32
    out = out.to(dtype)
    return out.flip(-1) if mirror else out


@pytest.fixture(scope="module")
def small(gpu, ccmi_lib):
    from ccmi import decode
    data = [_generate(21, 37, 7), _generate(34, 66, 9), _generate(21, 37, 11, generic=True)]
    plan = decode.roi_plan(data, (0, 0, 8, 8), output_chroma_format=444)
    assert [p["windowed"] for p in plan] == [True, True, False]  # the third takes the per-frame tail
    return data


@pytest.fixture(scope="module")
def small_ref(small):
    """{(bitdepth, chroma): [planes of every generated stream]} from decode_batch."""
    from ccmi import decode
    ref = {}
    for bitdepth, chroma in ((8, 420), (8, 444), (10, 444)):
        outs = decode.decode_batch(small, output_bitdepth=bitdepth, output_chroma_format=chroma, as_yuv=True)
        ref[(bitdepth, chroma)] = [_planes(r, h, w, bitdepth, chroma) for r, (h, w) in zip(outs, SMALL)]
    return ref


@pytest.fixture(scope="module")
def small_store(small):
    from ccmi import decode
    st = decode.LatentStore(small)
    yield st
    st.close()


def _ws(store, fill, **kw):
    import torch
    need = store.render_model_workspace_bytes(**kw)
    return torch.full((max(need, 256),), fill, dtype=torch.uint8, device="cuda")


def test_identity_equals_the_call_without_a_size(small, small_store, small_ref):
    """Region 8 x 8 -> 8 x 8: both passes are the identity, so the result is render_model's without
    a size, bit for bit -- on the window tail and on the per-frame tail, from streams and store."""
    from ccmi import decode
    rect, index = (3, 5, 8, 8), [0, 1, 2]
    for dtype in _dtypes():
        plain = small_store.render_model(index=index, roi=rect, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        sized = small_store.render_model(index=index, roi=rect, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444,
                                         size=(8, 8))
        coded = decode.decode_batch_model(small, roi=rect, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444,
                                          size=(8, 8))
        assert tuple(sized.shape) == (3, 3, 8, 8)
        for j in index:
            _same(sized[j], plain[j], ("store", dtype, j))
            _same(coded[j], plain[j], ("coded", dtype, j))
            _same(sized[j], _want(j, small_ref[(8, 444)][j], rect, (8, 8), mean=MEAN, std=STD, dtype=dtype), ("ref", dtype, j))


# (rect x y w h, size out_h out_w): the 21 x 37 frames (window tail: stream 0; per-frame cropping tail: 2)
CASES_444 = (
    ((1, 1, 36, 20), (7, 5)),     # non-integer downscale, odd origin, touches the right and bottom edges
    ((27, 15, 10, 6), (16, 23)),  # upscale, odd origin, the frame's bottom-right corner
    ((0, 0, 5, 21), (30, 2)),     # up on one axis, down on the other; left, top and bottom edges
    ((3, 2, 9, 7), (1, 1)),       # O = 1 on both axes
    ((36, 20, 1, 1), (5, 3)),     # I = 1: a 1 x 1 region
    ((0, 3, 37, 1), (4, 37)),     # one row, identity across, 4 rows out of 1
    ((5, 0, 1, 21), (21, 6)),     # one column, identity down
)


@pytest.mark.parametrize("rect,size", CASES_444)
def test_regions_444(small, small_store, small_ref, rect, size):
    from ccmi import decode
    for k, dtype in enumerate(_dtypes()):
        bitdepth = (8, 10, 8)[k]
        colour = ("rgb", "asis")[k % 2]
        planes = small_ref[(bitdepth, 444)]
        kw = dict(roi=rect, size=size, colour=colour, mean=MEAN, std=STD, dtype=dtype, output_bitdepth=bitdepth,
                  output_chroma_format=444)
        got = decode.decode_batch_model([small[0], small[2]], **kw)
        ren = small_store.render_model(index=[0, 2], **kw)
        assert tuple(got.shape) == tuple(ren.shape) == (2, 3) + size
        for j, i in enumerate((0, 2)):
            want = _want(i, planes[i], rect, size, bitdepth, 444, colour, MEAN, STD, dtype)
            _same(got[j], want, ("decode", rect, size, dtype, i))
            _same(ren[j], want, ("render", rect, size, dtype, i))


def test_whole_frame_down_on_one_axis_up_on_the_other(small, small_store, small_ref):
    """Region 34 x 66 -> 50 x 9, the whole frame: the batched whole-frame tail (no windows)."""
    from ccmi import decode
    rect, size = (0, 0, 66, 34), (50, 9)
    for dtype in _dtypes():
        got = decode.decode_batch_model([small[1]], size=size, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        _same(got[0], _want(1, small_ref[(8, 444)][1], rect, size, mean=MEAN, std=STD, dtype=dtype), dtype)
    # the generic 21 x 37 stream's whole frame: the per-frame tail without a crop
    ren = small_store.render_model(index=[2, 0], size=(10, 50), colour="asis", output_chroma_format=444)
    for j, i in enumerate((2, 0)):
        _same(ren[j], _want(i, small_ref[(8, 444)][i], (0, 0, 37, 21), (10, 50), colour="asis"), i)


@pytest.mark.parametrize("rect,size", (((2, 4, 6, 10), (7, 5)), ((10, 0, 56, 34), (17, 33)), ((64, 32, 2, 2), (3, 3)),
                                       ((0, 0, 66, 34), (1, 9))))
def test_420_even_rects_and_odd_output_sizes(small, small_store, small_ref, rect, size):
    """The 34 x 66 stream at its own 420: chroma from the even row and column, upsampled, then
    resampled; the evenness rule binds the region only."""
    from ccmi import decode
    planes = small_ref[(8, 420)][1]
    for k, dtype in enumerate(_dtypes()):
        colour = ("asis", "rgb")[k % 2]
        want = _want(1, planes, rect, size, 8, 420, colour, MEAN, STD, dtype)
        got = decode.decode_batch_model([small[1]], roi=rect, size=size, colour=colour, mean=MEAN, std=STD, dtype=dtype)
        _same(got[0], want, ("decode", rect, dtype))
        ren = small_store.render_model(index=[1], roi=rect, size=size, colour=colour, mean=MEAN, std=STD, dtype=dtype)
        _same(ren[0], want, ("render", rect, dtype))


def test_class_d_whole_frame_to_32x32(gpu, ccmi_lib):
    """One committed class-D stream, 416 x 240 -> 32 x 32 at 420: 25 and 15 taps per output sample."""
    import torch
    from ccmi import decode
    f = sorted((GOLDEN / "cool").glob("D-*.cool"))[0]
    data = [f.read_bytes()]
    planes = _planes(decode.decode_batch(data, as_yuv=True)[0], 240, 416, 8, 420)
    assert R.max_taps(416, 32) == 25 and R.max_taps(240, 32) == 15
    for dtype in (torch.float32, torch.bfloat16):
        got = decode.decode_batch_model(data, size=(32, 32), mean=MEAN, std=STD, dtype=dtype)
        assert decode.last_tail_groups() == (1, 0)
        _same(got[0], _want("D", planes, (0, 0, 416, 240), (32, 32), 8, 420, "rgb", MEAN, STD, dtype), dtype)


MIXED = ([0, 1, 0, 1, 0, 1],
         [(1, 1, 36, 20), (10, 3, 50, 30), (27, 15, 10, 6), (0, 0, 7, 34), (3, 2, 9, 7), (65, 33, 1, 1)])


def test_mixed_region_sizes_share_one_tail_group(small, small_store, small_ref):
    """Six frames of the two windowed streams, six region sizes, one output size: each equals its
    own single-frame reference, and the tail ran as ONE batched group, not one per size.  Adding
    the generic stream adds per-frame tails only.  Without a size, frames group by region size."""
    import torch
    from ccmi import decode
    index, rects = MIXED
    size = (12, 10)
    planes = small_ref[(8, 444)]
    for dtype in _dtypes():
        got = small_store.render_model(index=index, roi=rects, size=size, mean=MEAN, std=STD, dtype=dtype,
                                       output_chroma_format=444)
        assert decode.last_tail_groups() == (1, 0)
        for j, (i, r) in enumerate(zip(index, rects)):
            _same(got[j], _want(i, planes[i], r, size, mean=MEAN, std=STD, dtype=dtype), (dtype, j))
    got = decode.decode_batch_model([small[i] for i in index], roi=rects, size=size, dtype=torch.float16,
                                    output_chroma_format=444)
    assert decode.last_tail_groups() == (1, 0)
    for j, (i, r) in enumerate(zip(index, rects)):
        _same(got[j], _want(i, planes[i], r, size, dtype=torch.float16), ("coded", j))
    more = small_store.render_model(index=index + [2, 2], roi=rects + [(1, 1, 36, 20), (5, 0, 1, 21)], size=size,
                                    output_chroma_format=444)
    assert decode.last_tail_groups() == (1, 2)
    _same(more[6], _want(2, planes[2], (1, 1, 36, 20), size), "generic 6")
    _same(more[7], _want(2, planes[2], (5, 0, 1, 21), size), "generic 7")
    for j in range(6):
        _same(more[j], _want(index[j], planes[index[j]], rects[j], size), ("with generic", j))
    # the call without a size: two region sizes are two groups (and would not stack)
    small_store.render_model(index=[0, 1, 0, 1], roi=[(0, 0, 8, 8), (2, 2, 8, 8), (1, 1, 8, 8), (4, 4, 8, 8)],
                             output_chroma_format=444)
    assert decode.last_tail_groups() == (1, 0)
    with pytest.raises(ValueError, match="one size.*size="):
        small_store.render_model(index=[0, 1], roi=[(0, 0, 8, 8), (2, 2, 6, 8)], output_chroma_format=444)
    small_store.render(index=[0, 1], roi=[(0, 0, 8, 8), (2, 2, 6, 8)], output_chroma_format=444)
    assert decode.last_tail_groups() == (2, 0)


def test_layouts_and_mirror(small, small_store, small_ref):
    """NCHW, channels_last and mirror flags per frame, on mixed region sizes; output widths 10 (full
    and partial groups of 4) and 3."""
    import torch
    from ccmi import decode
    index, rects = MIXED
    flags = [True, False, False, True, True, False]
    planes = small_ref[(8, 444)]
    for size in ((12, 10), (5, 3)):
        for dtype in _dtypes():
            for cl in (False, True):
                got = small_store.render_model(index=index, roi=rects, size=size, mean=MEAN, std=STD, dtype=dtype,
                                               mirror=flags, channels_last=cl, output_chroma_format=444)
                assert tuple(got.shape) == (6, 3) + size
                if cl:
                    assert tuple(got.stride()) == (size[0] * size[1] * 3, 1, size[1] * 3, 3)
                for j, (i, r, m) in enumerate(zip(index, rects, flags)):
                    _same(got[j], _want(i, planes[i], r, size, mean=MEAN, std=STD, dtype=dtype, mirror=m), (size, dtype, cl, j))
    dec = decode.decode_batch_model([small[0], small[2]], roi=(1, 1, 36, 20), size=(7, 5), mirror=[False, True],
                                    channels_last=True, dtype=torch.bfloat16, output_chroma_format=444)
    for j, i in enumerate((0, 2)):
        _same(dec[j], _want(i, planes[i], (1, 1, 36, 20), (7, 5), dtype=torch.bfloat16, mirror=bool(j)), ("coded nhwc", j))


def test_out_views_into_a_canvas(small_store, small_ref):
    """Two 7 x 11 tiles written into a [3, 20, 40] canvas at different offsets from regions of two
    sizes: the tiles hold the frames, every other element still holds the sentinel."""
    planes = small_ref[(8, 444)]
    rects = [(1, 1, 36, 20), (27, 15, 10, 6)]
    for dtype in _dtypes():
        canvas, pat = _sentinel_canvas((3, 20, 40), dtype)
        spots = ((1, 3), (12, 25))
        tiles = [canvas[:, y: y + 7, x: x + 11] for y, x in spots]
        ret = small_store.render_model(index=[0, 2], roi=rects, size=(7, 11), out=tiles, mean=MEAN, std=STD, dtype=dtype,
                                       mirror=[True, False], output_chroma_format=444)
        assert ret[0] is tiles[0] and ret[1] is tiles[1]
        mask = np.ones((3, 20, 40), dtype=bool)
        for (y, x), i, r, m in zip(spots, (0, 2), rects, (True, False)):
            _same(canvas[:, y: y + 7, x: x + 11], _want(i, planes[i], r, (7, 11), mean=MEAN, std=STD, dtype=dtype, mirror=m),
                  (dtype, i))
            mask[:, y: y + 7, x: x + 11] = False
        assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), dtype


def test_out_tensors_take_the_output_size(small_store):
    import torch
    bad = [torch.zeros(3, 20, 36, device="cuda")]  # the region's size, not the output's
    with pytest.raises(ValueError, match="shape"):
        small_store.render_model(index=[0], roi=(1, 1, 36, 20), size=(7, 5), out=bad, output_chroma_format=444)
    with pytest.raises(ValueError, match="size"):
        small_store.render_model(index=[0], roi=(1, 1, 36, 20), size=(7, 5, 3), output_chroma_format=444)


@pytest.mark.parametrize("fill", (0xA5, 0x5A))
def test_decode_and_render_agree_on_a_prefilled_workspace(small, small_store, small_ref, fill):
    """decode_batch_model(size=) equals LatentStore.render_model(size=) bit for bit, and a render
    workspace prefilled with either byte gives the reference: nothing unwritten is read."""
    from ccmi import decode
    index, rects = MIXED
    index, rects = index + [2], rects + [(1, 1, 36, 20)]
    size = (9, 14)
    planes = small_ref[(8, 444)]
    for dtype in _dtypes():
        kw = dict(roi=rects, size=size, colour="asis", mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        a = decode.decode_batch_model([small[i] for i in index], **kw)
        ws = _ws(small_store, fill, index=index, roi=rects, size=size, output_chroma_format=444)
        b = small_store.render_model(index=index, workspace=ws, **kw)
        assert a.shape == b.shape and a.stride() == b.stride()
        assert np.array_equal(_bits(a), _bits(b)), dtype
        for j, (i, r) in enumerate(zip(index, rects)):
            _same(b[j], _want(i, planes[i], r, size, 8, 444, "asis", MEAN, STD, dtype), (fill, dtype, j))


def test_plan_errors_leave_the_destination_untouched(small_store):
    """An output size outside [1, 16384] through the GPU entry point: CcmiError naming the frame."""
    import torch
    from ccmi import CcmiError
    dst = [torch.full((3, 4, 4), 7.0, device="cuda")]
    for size in ((0, 4), (4, 16385)):
        with pytest.raises(CcmiError, match="frame 0.*output size"):
            small_store.render_model(index=[0], roi=(0, 0, 8, 8), size=size, out=dst, output_chroma_format=444)
    torch.cuda.synchronize()
    assert bool((dst[0] == 7.0).all())
