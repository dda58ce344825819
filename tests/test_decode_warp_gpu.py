"""Warped formatted output (ccmi_decode_batch_dev_warp / ccmi_latents_render_warp;
decode.decode_batch_model(affine=...) and LatentStore.render_model(affine=...)): every output pixel
a bilinear sample of the decoded frame through the frame's own 2 x 3 matrix, in the decoder's
output stage, and frames with any matrices sharing the tail's launches.

The reference is never the new code: the bytes of decode.decode_batch, split into planes, steps
1-3 of the ccmi_tensor_fmt contract over the WHOLE frame restated with torch CPU float32 operations
as tests/test_decode_fmt_gpu.py does, steps 3a-3d in numpy float32 one rounded operation at a time
(tests/warp_ref.py, pinned by tests/test_decode_warp_ref.py), then scale, bias and .to(dtype).
Every comparison is BITWISE for float32, float16 and bfloat16.

The streams are the formatted-output tests': 21 x 37, 34 x 66 and 21 x 37 with a generic synthesis
(per-frame tail), generated; and one committed class-D 416 x 240 stream.  Every render from the
store runs twice, on a workspace prefilled with 0xA5 and with 0x5A, and must give the same bits: a
read outside what the tail wrote for the window shows as a difference."""
import math
from pathlib import Path

import numpy as np
import pytest

import warp_ref as W
from test_decode_fmt_gpu import MEAN, SMALL, STD, YUV2RGB, _bits, _f32, _generate, _planes, _same, _sentinel_canvas

GOLDEN = Path(__file__).resolve().parent / "golden"
FILL = (0.2, 0.5, 0.7)
PADS = {"fill": W.PAD_FILL, "edge": W.PAD_EDGE}

pytestmark = pytest.mark.gpu


def _dtypes():
    import torch
    return (torch.float32, torch.float16, torch.bfloat16)


_Q = {}


def _q(key, planes, bitdepth, chroma, colour, yuv=True):
    """Steps 1-3 over the whole frame (torch CPU float32): [3, H, W] float32, computed once per
    (stream, format) and shared, read-only."""
    import torch
    k = (key, bitdepth, chroma, colour)
    if k not in _Q:
        s = [torch.from_numpy(np.ascontiguousarray(p).astype(np.int32)) for p in planes]
        if chroma == 420:
            s = [s[0]] + [p.repeat_interleave(2, 0).repeat_interleave(2, 1) for p in s[1:]]
        assert s[1].shape == s[0].shape == s[2].shape
        maxv = float((1 << bitdepth) - 1)
        p = [t.to(torch.float32) / maxv for t in s]
        q = p
        if colour == "rgb" and yuv:
            q = []
            for a, b, o in YUV2RGB:
                a, b, o = _f32(a), _f32(b), _f32(o / 255.0)
                q.append((((p[0] + a * p[1]) + b * p[2]) + o).clamp(0.0, 1.0))
        q = torch.stack(q).numpy()
        assert q.dtype == np.float32
        q.setflags(write=False)
        _Q[k] = q
    return _Q[k]


def _want(q, m, size, pad="fill", fill=0.0, mean=None, std=None, dtype=None, mirror=False):
    import torch
    dtype = dtype or torch.float32
    r = torch.from_numpy(W.warp(q, m, size[0], size[1], PADS[pad], fill))
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    out = torch.stack([r[c] * _f32(1.0 / std[c]) + _f32(-mean[c] / std[c]) for c in range(3)])
    assert out.dtype == torch.float32
    out = out.to(dtype)
    return out.flip(-1) if mirror else out


def _mat(A, centre, size):
    """The matrix with linear part A that maps the centre of the size = (out_h, out_w) output to centre = (x, y)."""
    A = np.asarray(A, np.float64).reshape(2, 2)
    t = np.asarray(centre, np.float64) - A @ np.array([size[1] / 2, size[0] / 2])
    return np.array([A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1]], np.float32)


def _rot(deg, scale=1.0):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s], [s, c]]) / scale


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


def _render(store, **kw):
    """store.render_model(**kw) on a workspace prefilled with 0xA5, then with 0x5A: the same bits."""
    import torch
    plan = {k: kw[k] for k in ("index", "size", "affine", "pad", "fill", "roi", "output_bitdepth", "output_chroma_format")
            if k in kw}
    need = store.render_model_workspace_bytes(**plan)
    outs = []
    for fill in (0xA5, 0x5A):
        ws = torch.full((max(need, 256),), fill, dtype=torch.uint8, device="cuda")
        outs.append(store.render_model(workspace=ws, **kw))
    a, b = outs
    if isinstance(a, list):
        a, b = torch.stack([t.contiguous() for t in a]), torch.stack([t.contiguous() for t in b])
    assert np.array_equal(_bits(a), _bits(b)), "the result depends on what the workspace held"
    return outs[1]


def test_identity_and_integer_translation_are_the_crop(small, small_store, small_ref):
    """m = 1 0 x / 0 1 y equals render_model(roi=(x, y, w, h)) bit for bit: from the store and from
    coded streams, on the window tail (streams 0, 1) and on the per-frame tail (2)."""
    from ccmi import decode
    index = [0, 1, 2]
    for k, (x, y, w, h) in enumerate(((0, 0, 8, 8), (3, 5, 8, 8), (29, 13, 8, 8), (5, 0, 7, 21), (36, 20, 1, 1))):
        dtype = _dtypes()[k % 3]
        m = np.array([1, 0, x, 0, 1, y], np.float32)
        kw = dict(mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        plain = small_store.render_model(index=index, roi=(x, y, w, h), **kw)
        warped = _render(small_store, index=index, affine=m.reshape(2, 3), size=(h, w), **kw)
        coded = decode.decode_batch_model(small, affine=[m.reshape(2, 3)] * 3, size=(h, w), pad="edge", **kw)
        assert tuple(warped.shape) == (3, 3, h, w)
        for j in index:
            _same(warped[j], plain[j], ("store", dtype, j, x, y))
            _same(coded[j], plain[j], ("coded", dtype, j, x, y))
            q = _q(j, small_ref[(8, 444)][j], 8, 444, "rgb")
            _same(warped[j], _want(q, m, (h, w), mean=MEAN, std=STD, dtype=dtype), ("ref", dtype, j, x, y))
    # the whole frame: the whole-frame tail, batched (stream 1) and per frame (stream 2)
    for j in (1, 2):
        h, w = SMALL[j]
        got = _render(small_store, index=[j], affine=[[1, 0, 0], [0, 1, 0]], size=(h, w), output_chroma_format=444)
        assert small_store.warp_plan([j], [[1, 0, 0], [0, 1, 0]], (h, w), output_chroma_format=444)[0]["window"] == (0, 0, w, h)
        _same(got[0], small_store.render_model(index=[j], output_chroma_format=444)[0], ("whole", j))
    # 420 on the 34 x 66 stream: an even translation is the 420 crop, m00 = -1 its flip
    plain = small_store.render_model(index=[1], roi=(10, 4, 12, 8), mean=MEAN, std=STD)
    got = _render(small_store, index=[1, 1], affine=[[[1, 0, 10], [0, 1, 4]], [[-1, 0, 22], [0, 1, 4]]], size=(8, 12),
                  mean=MEAN, std=STD)
    _same(got[0], plain[0], "420 crop")
    _same(got[1], plain[0].flip(-1), "420 flip")


KINDS = {"rot30": _rot(30), "rot90": np.array([[0, -1], [1, 0]]), "scale0.5": np.eye(2) * 2, "scale2": np.eye(2) * 0.5,
         "singular": np.zeros((2, 2))}
# centres in the 21 x 37 frame (x, y): inside, on each edge, on each corner, wholly outside
PLACES = ((18.3, 10.6), (0, 10.5), (37, 10.5), (18.5, 0), (18.5, 21), (0, 0), (37, 0), (0, 21), (37, 21), (-70.2, -60.7))
SIZES = ((1, 1), (8, 8), (16, 24))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rotation_scale_and_singular_matrices(small, small_store, small_ref, kind):
    """Every placement, both pads and three output sizes, on the window tail (stream 0) and on the
    per-frame tail (stream 2), one call per (size, pad)."""
    import torch
    from ccmi import decode
    planes = small_ref[(8, 444)]
    index = [0] * len(PLACES) + [2] * len(PLACES)
    calls = 0
    for size in SIZES:
        mats = np.stack([_mat(KINDS[kind], c, size) for c in PLACES] * 2)
        for pad in ("fill", "edge"):
            dtype = _dtypes()[calls % 3]
            calls += 1
            kw = dict(affine=mats.reshape(-1, 2, 3), size=size, pad=pad, fill=FILL, mean=MEAN, std=STD, dtype=dtype,
                      output_chroma_format=444)
            got = _render(small_store, index=index, **kw)
            # a window that covers the frame (scale 0.5 at 16 x 24) runs the whole-frame tail: a group of its own
            groups = decode.last_tail_groups()
            assert groups[1] == len(PLACES) and 1 <= groups[0] <= 2, groups
            for j, (i, m) in enumerate(zip(index, mats)):
                q = _q(i, planes[i], 8, 444, "rgb")
                _same(got[j], _want(q, m, size, pad, FILL, MEAN, STD, dtype), (kind, size, pad, dtype, j))
            if size == (8, 8):  # the same from coded streams
                coded = decode.decode_batch_model([small[i] for i in index], **kw)
                assert np.array_equal(_bits(coded), _bits(got)), (kind, pad)
    # wholly outside: all fill, or the nearest corner pixel
    far = _mat(KINDS[kind], PLACES[-1], (8, 8)).reshape(2, 3)
    out = _render(small_store, index=[0], affine=far, size=(8, 8), pad="fill", fill=FILL, output_chroma_format=444)
    q = _q(0, planes[0], 8, 444, "rgb")
    _same(out[0], _want(q, far, (8, 8), "fill", FILL), (kind, "outside, fill"))
    # the blend of four equal taps t is (t (1 - f)) + (t f): t but for the roundings of 1 - f, the two products and the sum
    assert bool(((out[0].cpu() - torch.tensor(FILL)[:, None, None]).abs() <= 4 * 2.0 ** -24).all())
    edge = _render(small_store, index=[0], affine=far, size=(8, 8), pad="edge", output_chroma_format=444)
    _same(edge[0], _want(q, far, (8, 8), "edge"), (kind, "outside, edge"))
    corner = small_store.render_model(index=[0], roi=(0, 0, 1, 1), output_chroma_format=444)[0]
    assert bool(((edge[0] - corner).abs() <= 4 * 2.0 ** -24).all())


def test_taps_on_integer_positions_and_the_last_row_and_column(small_store, small_ref):
    """u = -1, 0, W - 1 (fx = 0: the second tap has weight 0 but is still read or padded) and the
    half positions between; v alike."""
    planes = small_ref[(8, 444)]
    H, Wd = SMALL[0]
    size = (6, 5)
    offs_x = (-1, 0, -0.5, Wd - 1 - 4, Wd - 4, Wd - 4.5)   # u of column k = k + off
    offs_y = (-1, 0, -0.5, H - 1 - 5, H - 5, H - 5.5)
    mats = [np.array([1, 0, ox, 0, 1, oy], np.float32) for ox in offs_x for oy in offs_y]
    for i in (0, 2):
        for k, pad in enumerate(("fill", "edge")):
            dtype = _dtypes()[(i + k) % 3]
            got = _render(small_store, index=[i] * len(mats), affine=np.stack(mats).reshape(-1, 2, 3), size=size, pad=pad,
                          fill=FILL, dtype=dtype, colour="asis", output_chroma_format=444)
            q = _q(i, planes[i], 8, 444, "asis")
            for j, m in enumerate(mats):
                _same(got[j], _want(q, m, size, pad, FILL, dtype=dtype), (i, pad, j))


def test_sample_formats_colour_and_mirror(small, small_store, small_ref):
    """420 (the 34 x 66 stream: chroma at the even row and column of the FRAME) and 444, 8 and 10
    bits, 'rgb' and 'asis', mirror flags per frame."""
    from ccmi import decode
    size = (16, 24)
    places = ((30.2, 17.4), (0, 0), (66, 34), (65.5, 10), (-90, 5))
    flags = [True, False, True, False, True]
    for k, (bitdepth, chroma, colour) in enumerate(((8, 420, "rgb"), (8, 420, "asis"), (10, 444, "rgb"), (10, 444, "asis"),
                                                    (8, 444, "rgb"))):
        dtype = _dtypes()[k % 3]
        pad = ("edge", "fill")[k % 2]
        mats = np.stack([_mat(_rot(30, 0.8), c, size) for c in places])
        kw = dict(affine=mats.reshape(-1, 2, 3), size=size, pad=pad, fill=FILL, colour=colour, mean=MEAN, std=STD, dtype=dtype,
                  mirror=flags, output_bitdepth=bitdepth, output_chroma_format=chroma)
        got = _render(small_store, index=[1] * len(places), **kw)
        q = _q(1, small_ref[(bitdepth, chroma)][1], bitdepth, chroma, colour)
        for j, m in enumerate(mats):
            _same(got[j], _want(q, m, size, pad, FILL, MEAN, STD, dtype, mirror=flags[j]), (bitdepth, chroma, colour, j))
        if k in (0, 3):
            coded = decode.decode_batch_model([small[1]] * len(places), **kw)
            assert np.array_equal(_bits(coded), _bits(got)), (bitdepth, chroma, colour)
    # the plan's windows at 420 are even
    for p in small_store.warp_plan([1] * len(places), mats.reshape(-1, 2, 3), size):
        assert all(v % 2 == 0 for v in p["window"]) and p["windowed"]
    # 420 samples of an odd frame are refused; 444 takes them
    from ccmi import CcmiError
    with pytest.raises(CcmiError, match="frame 0.*even"):
        small_store.render_model(index=[0], affine=mats[0].reshape(2, 3), size=size)


def test_class_d_and_kodak(gpu, ccmi_lib):
    """One committed class-D stream (416 x 240, 420) and one Kodak stream (RGB: no matrix), rotated
    views at the frame's corners and inside it."""
    import torch
    from ccmi import decode
    f = sorted((GOLDEN / "cool").glob("D-*.cool"))[0]
    data = [f.read_bytes()]
    planes = _planes(decode.decode_batch(data, as_yuv=True)[0], 240, 416, 8, 420)
    q = _q("D", planes, 8, 420, "rgb")
    size = (16, 24)
    places = ((200.3, 120.9), (0, 0), (416, 240), (416, 3.5), (5.5, 240))
    mats = np.stack([_mat(_rot(-30, s), c, size) for c, s in zip(places, (0.5, 1.0, 2.0, 0.7, 1.5))])
    for dtype, pad in ((torch.float32, "fill"), (torch.bfloat16, "edge")):
        got = decode.decode_batch_model(data * len(places), affine=mats.reshape(-1, 2, 3), size=size, pad=pad, fill=FILL,
                                        mean=MEAN, std=STD, dtype=dtype)
        assert decode.last_tail_groups() == (1, 0)
        for j, m in enumerate(mats):
            _same(got[j], _want(q, m, size, pad, FILL, MEAN, STD, dtype), ("D", dtype, j))
    crop = decode.decode_batch_model(data, roi=(100, 60, 24, 16), dtype=torch.float16)
    same = decode.decode_batch_model(data, affine=[[1, 0, 100], [0, 1, 60]], size=size, dtype=torch.float16)
    _same(same[0], crop[0], "D crop")
    kod = sorted((GOLDEN / "cool").rglob("kodim*.cool"))
    if not kod:
        return
    kdata = kod[0].read_bytes()
    geom, _ = decode.decode_batch_geometry([kdata])
    h, w = geom[0]["height"], geom[0]["width"]
    ppm, = decode.decode_batch([kdata], as_yuv=False)
    hdr = b"P6\n%d %d\n255\n" % (w, h)
    kplanes = list(np.frombuffer(ppm[len(hdr):], dtype="u1").reshape(h, w, 3).transpose(2, 0, 1))
    kq = _q("kodak", kplanes, 8, 444, "rgb", yuv=False)
    km = np.stack([_mat(_rot(30, 0.6), c, size) for c in ((w - 3.5, h - 2.2), (w / 2, h / 2))])
    got = decode.decode_batch_model([kdata] * 2, affine=km.reshape(-1, 2, 3), size=size, pad="fill", fill=FILL, mean=MEAN,
                                    std=STD, dtype=torch.bfloat16)
    for j, m in enumerate(km):
        _same(got[j], _want(kq, m, size, "fill", FILL, MEAN, STD, torch.bfloat16), ("kodak", j))


def test_layouts_and_a_view_into_a_canvas(small_store, small_ref):
    """NCHW, channels_last (output widths 24: full groups of 4; 7 and 3: partial ones), and tiles of
    a sentinel canvas: nothing outside the tiles changes."""
    planes = small_ref[(8, 444)]
    index = [0, 2, 0, 2]
    flags = [False, True, True, False]
    for size in ((16, 24), (5, 7), (2, 3)):
        mats = np.stack([_mat(_rot(30 * (j + 1), 1.25), (4.0 + 9 * j, 3.0 + 5 * j), size) for j in range(4)])
        for dtype in _dtypes():
            for cl in (False, True):
                got = _render(small_store, index=index, affine=mats.reshape(-1, 2, 3), size=size, pad="edge", mean=MEAN,
                              std=STD, dtype=dtype, mirror=flags, channels_last=cl, output_chroma_format=444)
                assert tuple(got.shape) == (4, 3) + size
                if cl:
                    assert tuple(got.stride()) == (size[0] * size[1] * 3, 1, size[1] * 3, 3)
                for j, (i, m) in enumerate(zip(index, mats)):
                    q = _q(i, planes[i], 8, 444, "rgb")
                    _same(got[j], _want(q, m, size, "edge", 0.0, MEAN, STD, dtype, mirror=flags[j]), (size, dtype, cl, j))
    size = (7, 11)
    mats = np.stack([_mat(_rot(30), (2.0, 3.0), size), _mat(_rot(-45, 2.0), (30.0, 18.0), size)])
    for dtype in _dtypes():
        canvas, pat = _sentinel_canvas((3, 20, 40), dtype)
        spots = ((1, 3), (12, 25))
        tiles = [canvas[:, y: y + 7, x: x + 11] for y, x in spots]
        ret = small_store.render_model(index=[0, 2], affine=mats.reshape(-1, 2, 3), size=size, out=tiles, fill=FILL, mean=MEAN,
                                       std=STD, dtype=dtype, mirror=[True, False], output_chroma_format=444)
        assert ret[0] is tiles[0] and ret[1] is tiles[1]
        mask = np.ones((3, 20, 40), dtype=bool)
        for (y, x), i, m, mir in zip(spots, (0, 2), mats, (True, False)):
            q = _q(i, planes[i], 8, 444, "rgb")
            _same(canvas[:, y: y + 7, x: x + 11], _want(q, m, size, "fill", FILL, MEAN, STD, dtype, mirror=mir), (dtype, i))
            mask[:, y: y + 7, x: x + 11] = False
        assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), dtype


def test_64_frames_with_random_matrices_share_one_tail_group(small, small_store, small_ref):
    """64 frames over the three generated streams, random rotation / scale / centre each, ONE call:
    every frame equals its own reference, and the tail ran as one batched group plus one per-frame
    tail for each frame of the generic-synthesis stream."""
    import torch
    from ccmi import decode
    rng = np.random.default_rng(11)
    size = (8, 8)
    index = [int(v) for v in rng.integers(0, 3, 64)]
    mats = []
    for i in index:
        H, Wd = SMALL[i]
        A = _rot(rng.uniform(-180, 180), rng.uniform(0.6, 1.5))
        mats.append(_mat(A, (rng.uniform(-4, Wd + 4), rng.uniform(-4, H + 4)), size))
    mats = np.stack(mats)
    k = index.count(2)
    assert 0 < k < 64 and index.count(0) and index.count(1)
    planes = small_ref[(8, 444)]
    flags = [bool(v) for v in rng.integers(0, 2, 64)]
    for dtype, pad in ((torch.bfloat16, "fill"), (torch.float32, "edge")):
        kw = dict(affine=mats.reshape(-1, 2, 3), size=size, pad=pad, fill=FILL, mean=MEAN, std=STD, dtype=dtype, mirror=flags,
                  output_chroma_format=444)
        got = _render(small_store, index=index, **kw)
        assert decode.last_tail_groups() == (1, k)
        for j, (i, m) in enumerate(zip(index, mats)):
            q = _q(i, planes[i], 8, 444, "rgb")
            _same(got[j], _want(q, m, size, pad, FILL, MEAN, STD, dtype, mirror=flags[j]), (dtype, j, i))
    # from coded streams the ARM decode runs in chunks, each with its own tail: a group per chunk
    coded = decode.decode_batch_model([small[i] for i in index], **kw)
    assert decode.last_tail_groups()[1] == k
    assert np.array_equal(_bits(coded), _bits(got))


def test_python_arguments(small, small_store):
    from ccmi import decode
    m = [[1, 0, 0], [0, 1, 0]]
    with pytest.raises(ValueError, match="size"):
        small_store.render_model(index=[0], affine=m, output_chroma_format=444)
    with pytest.raises(ValueError, match="roi"):
        small_store.render_model(index=[0], affine=m, size=(4, 4), roi=(0, 0, 4, 4), output_chroma_format=444)
    with pytest.raises(ValueError, match="roi"):
        decode.decode_batch_model(small[:1], affine=m, size=(4, 4), roi=(0, 0, 4, 4), output_chroma_format=444)
    with pytest.raises(ValueError, match="pad"):
        small_store.render_model(index=[0], affine=m, size=(4, 4), pad="wrap", output_chroma_format=444)
    with pytest.raises(ValueError, match="affine"):
        small_store.render_model(index=[0, 1], affine=[m] * 3, size=(4, 4), output_chroma_format=444)
    with pytest.raises(ValueError, match="fill"):
        small_store.render_model(index=[0], affine=m, size=(4, 4), fill=(0.1, 0.2), output_chroma_format=444)
    import torch
    a = small_store.render_model(index=[0, 1], affine=torch.tensor(m), size=(4, 4), output_chroma_format=444)
    b = small_store.render_model(index=[0, 1], affine=np.array([m, m]), size=(4, 4), fill=0.0, output_chroma_format=444)
    assert np.array_equal(_bits(a), _bits(b))
    plan = small_store.warp_plan([0, 2], m, (4, 4), output_chroma_format=444)
    assert [p["window"] for p in plan] == [(0, 0, 6, 6)] * 2 and [p["windowed"] for p in plan] == [True, False]
    assert len(plan[0]["arm_rows"]) == len(small_store.roi_plan([0], (0, 0, 6, 6), output_chroma_format=444)[0]["arm_rows"])
    assert plan[0]["arm_rows"] == small_store.roi_plan([0], (0, 0, 6, 6), output_chroma_format=444)[0]["arm_rows"]


def test_plan_errors_leave_the_destination_untouched(small_store):
    import torch
    from ccmi import CcmiError
    dst = [torch.full((3, 4, 4), 7.0, device="cuda")]
    for m, what in (([[float("nan"), 0, 0], [0, 1, 0]], "finite"), ([[1, 0, 5e6], [0, 1, 0]], "2\\^22")):
        with pytest.raises(CcmiError, match="frame 0.*" + what):
            small_store.render_model(index=[0], affine=m, size=(4, 4), out=dst, output_chroma_format=444)
    torch.cuda.synchronize()
    assert bool((dst[0] == 7.0).all())


def test_the_unchanged_calls_return_what_they_did(small_store, small_ref):
    """render_model with and without size=, against the resample tests' reference."""
    from test_decode_resample_gpu import _want as want_rs
    planes = small_ref[(8, 444)]
    for dtype in _dtypes():
        plain = small_store.render_model(index=[0, 2], roi=(3, 5, 8, 8), mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        sized = small_store.render_model(index=[0, 2], roi=(1, 1, 36, 20), size=(7, 5), mean=MEAN, std=STD, dtype=dtype,
                                         output_chroma_format=444)
        for j, i in enumerate((0, 2)):
            _same(plain[j], want_rs(i, planes[i], (3, 5, 8, 8), (8, 8), mean=MEAN, std=STD, dtype=dtype), ("plain", dtype, i))
            _same(sized[j], want_rs(i, planes[i], (1, 1, 36, 20), (7, 5), mean=MEAN, std=STD, dtype=dtype), ("sized", dtype, i))
