"""Bicubic interpolation in the resize and the warp of the decoder's output stage
(CCMI_FILTER_CUBIC / CCMI_WARP_CUBIC and their clamp flags; interpolation="bicubic" and clamp= of
decode.decode_batch_model and LatentStore.render_model).

The reference is never the new code: the bytes of decode.decode_batch, split into planes, steps 1-3
of the ccmi_tensor_fmt contract over the WHOLE frame restated with torch CPU float32 operations
(tests/test_decode_warp_gpu.py's _q), the cubic steps in numpy float32 one rounded operation at a
time (tests/cubic_ref.py, pinned by tests/test_decode_cubic_ref.py), the later stages through
tests/colour_ref.py, tests/tone_ref.py and tests/filter_ref.py, then scale, bias and .to(dtype).
Every comparison is BITWISE for float32, float16 and bfloat16.  The warp reference samples the whole
decoded frame, so a window that is too small shows as wrong values; every render from the store
runs on a workspace of exactly the planned bytes, prefilled with 0xA5 and then with 0x5A.

The streams are the formatted-output tests': 21 x 37 (window tail), 34 x 66 (420) and 21 x 37 with
a generic synthesis (per-frame tail), generated."""
import numpy as np
import pytest

import colour_ref as KR
import cubic_ref as R
import filter_ref as FR
import tone_ref as TR
from test_decode_fmt_gpu import MEAN, SMALL, STD, _bits, _f32, _generate, _planes, _same, _sentinel_canvas
from test_decode_warp_gpu import _mat, _q, _rot

FILL = (0.2, 0.5, 0.7)
PADS = {"fill": R.PAD_FILL, "edge": R.PAD_EDGE}

pytestmark = pytest.mark.gpu


def _dtypes():
    import torch
    return (torch.float32, torch.float16, torch.bfloat16)


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


PLAN_KEYS = ("index", "size", "affine", "pad", "fill", "roi", "output_bitdepth", "output_chroma_format", "interpolation",
             "clamp", "colour_ops", "blur", "solarize", "tone_ops")


def _render(store, **kw):
    """store.render_model(**kw) on a workspace of exactly the planned bytes, prefilled with 0xA5, then
    with 0x5A: the same bits (nothing unwritten is read, nothing past the plan is needed)."""
    import torch
    need = store.render_model_workspace_bytes(**{k: kw[k] for k in PLAN_KEYS if k in kw})
    outs = []
    for fill in (0xA5, 0x5A):
        ws = torch.full((max(need, 1),), fill, dtype=torch.uint8, device="cuda")
        outs.append(store.render_model(workspace=ws, **kw))
    a, b = outs
    if isinstance(a, list):
        a, b = torch.stack([t.contiguous() for t in a]), torch.stack([t.contiguous() for t in b])
    assert np.array_equal(_bits(a), _bits(b)), "the result depends on what the workspace held"
    return outs[1]


_GEO = {}


def _resized(key, q, rect, size, clamp=False):
    """r' of the cubic resize of q's region: [3, out_h, out_w] float32, computed once, read-only."""
    k = ("rs", key, rect, size, clamp)
    if k not in _GEO:
        x, y, w, h = rect
        r = R.resample(q[:, y: y + h, x: x + w], size[0], size[1], clamp=clamp)
        r.setflags(write=False)
        _GEO[k] = r
    return _GEO[k]


def _warped(key, q, m, size, pad="fill", fill=0.0, clamp=False):
    k = ("warp", key, tuple(float(v) for v in np.asarray(m).reshape(6)), size, pad, tuple(np.atleast_1d(fill).tolist()), clamp)
    if k not in _GEO:
        r = R.warp(q, m, size[0], size[1], PADS[pad], fill, clamp=clamp)
        r.setflags(write=False)
        _GEO[k] = r
    return _GEO[k]


def _finish(r, mean=None, std=None, dtype=None, mirror=False):
    """steps 4-6 on r' (an array or a CPU tensor)"""
    import torch
    dtype = dtype or torch.float32
    r = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.array(r))
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    out = torch.stack([r[c] * _f32(1.0 / std[c]) + _f32(-mean[c] / std[c]) for c in range(3)])
    assert out.dtype == torch.float32
    out = out.to(dtype)
    return out.flip(-1) if mirror else out


# ------------------------------------------------------------------ the resize
def test_identity_equals_the_call_without_a_size(small, small_store, small_ref):
    """8 x 8 -> 8 x 8: the neighbours' weights are exactly 0, so both passes are the identity."""
    from ccmi import decode
    rect, index = (3, 5, 8, 8), [0, 1, 2]
    for dtype in _dtypes():
        kw = dict(roi=rect, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        plain = small_store.render_model(index=index, **kw)
        sized = _render(small_store, index=index, size=(8, 8), interpolation="bicubic", **kw)
        coded = decode.decode_batch_model(small, size=(8, 8), interpolation="bicubic", clamp=True, **kw)
        for j in index:
            _same(sized[j], plain[j], ("store", dtype, j))
            _same(coded[j], plain[j], ("coded", dtype, j))


# (rect x y w h, size out_h out_w) on the 21 x 37 frames: stream 0 (window tail) and 2 (per-frame cropping tail)
CASES_444 = (
    ((0, 0, 37, 21), (8, 8)),    # the whole frame down: taps clipped at both edges of both axes
    ((3, 2, 3, 5), (1, 1)),      # 5 x 3 -> 1 x 1: every tap run clipped at both ends; output width 1
    ((0, 0, 37, 21), (20, 36)),  # near-identity: 37 -> 36 and 21 -> 20
    ((36, 20, 1, 1), (3, 5)),    # up from side 1; output width 5 (one full and one partial group of four)
    ((10, 4, 2, 3), (9, 7)),     # up from sides 2 and 3: the negative lobes, renormalised at the edges; width 7
    ((3, 5, 8, 8), (21, 37)),    # 8 x 8 -> 21 x 37
)


@pytest.mark.parametrize("rect,size", CASES_444)
def test_regions_444(small, small_store, small_ref, rect, size):
    from ccmi import decode
    for k, dtype in enumerate(_dtypes()):
        bitdepth, colour = (8, 10, 8)[k], ("rgb", "asis")[k % 2]
        kw = dict(roi=rect, size=size, colour=colour, mean=MEAN, std=STD, dtype=dtype, output_bitdepth=bitdepth,
                  output_chroma_format=444, interpolation="bicubic")
        got = decode.decode_batch_model([small[0], small[2]], **kw)
        ren = _render(small_store, index=[0, 2], **kw)
        assert tuple(got.shape) == tuple(ren.shape) == (2, 3) + size
        for j, i in enumerate((0, 2)):
            q = _q(i, small_ref[(bitdepth, 444)][i], bitdepth, 444, colour)
            want = _finish(_resized((i, bitdepth, 444, colour), q, rect, size), MEAN, STD, dtype)
            _same(got[j], want, ("decode", rect, size, dtype, i))
            _same(ren[j], want, ("render", rect, size, dtype, i))


@pytest.mark.parametrize("rect,size", (((2, 4, 6, 10), (7, 5)), ((10, 0, 56, 34), (17, 33)), ((0, 0, 66, 34), (50, 9))))
def test_420_even_regions(small, small_store, small_ref, rect, size):
    """The 34 x 66 stream at its own 420; the last case is the whole frame (the whole-frame tail)."""
    from ccmi import decode
    for k, dtype in enumerate(_dtypes()):
        colour = ("asis", "rgb")[k % 2]
        q = _q(1, small_ref[(8, 420)][1], 8, 420, colour)
        want = _finish(_resized((1, 8, 420, colour), q, rect, size), MEAN, STD, dtype)
        kw = dict(roi=rect, size=size, colour=colour, mean=MEAN, std=STD, dtype=dtype, interpolation="bicubic")
        _same(decode.decode_batch_model([small[1]], **kw)[0], want, ("decode", rect, dtype))
        _same(_render(small_store, index=[1], **kw)[0], want, ("render", rect, dtype))


MIXED = ([0, 1, 0, 1, 0, 1], [(1, 1, 36, 20), (10, 3, 50, 30), (27, 15, 10, 6), (0, 0, 7, 34), (3, 2, 9, 7), (65, 33, 1, 1)])


def test_mixed_region_sizes_share_one_tail_group(small, small_store, small_ref):
    """Six region sizes, one output size, one batched tail group -- as with the triangle; the generic
    stream adds per-frame tails only."""
    import torch
    from ccmi import decode
    index, rects = MIXED
    size = (12, 10)
    for dtype in _dtypes():
        kw = dict(roi=rects, size=size, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444, interpolation="bicubic")
        small_store.render_model(index=index, **{**kw, "interpolation": "bilinear"})
        bilinear_groups = decode.last_tail_groups()
        got = small_store.render_model(index=index, **kw)
        assert decode.last_tail_groups() == bilinear_groups == (1, 0)
        for j, (i, r) in enumerate(zip(index, rects)):
            q = _q(i, small_ref[(8, 444)][i], 8, 444, "rgb")
            _same(got[j], _finish(_resized((i, 8, 444, "rgb"), q, r, size), MEAN, STD, dtype), (dtype, j))
    more = decode.decode_batch_model([small[i] for i in index + [2]], roi=rects + [(5, 0, 1, 21)], size=size,
                                     dtype=torch.float16, output_chroma_format=444, interpolation="bicubic")
    assert decode.last_tail_groups() == (1, 1)
    for j, (i, r) in enumerate(zip(index + [2], rects + [(5, 0, 1, 21)])):
        q = _q(i, small_ref[(8, 444)][i], 8, 444, "rgb")
        _same(more[j], _finish(_resized((i, 8, 444, "rgb"), q, r, size), dtype=torch.float16), ("coded", j))


def test_layouts_mirror_and_views_into_a_canvas(small, small_store, small_ref):
    index, rects = MIXED
    flags = [True, False, False, True, True, False]
    for size in ((12, 10), (5, 3)):
        for dtype in _dtypes():
            for cl in (False, True):
                got = small_store.render_model(index=index, roi=rects, size=size, mean=MEAN, std=STD, dtype=dtype, mirror=flags,
                                               channels_last=cl, output_chroma_format=444, interpolation="bicubic")
                if cl:
                    assert tuple(got.stride()) == (size[0] * size[1] * 3, 1, size[1] * 3, 3)
                for j, (i, r, m) in enumerate(zip(index, rects, flags)):
                    q = _q(i, small_ref[(8, 444)][i], 8, 444, "rgb")
                    _same(got[j], _finish(_resized((i, 8, 444, "rgb"), q, r, size), MEAN, STD, dtype, m), (size, dtype, cl, j))
    rects = [(1, 1, 36, 20), (27, 15, 10, 6)]
    for dtype in _dtypes():
        canvas, pat = _sentinel_canvas((3, 20, 40), dtype)
        spots = ((1, 3), (12, 25))
        tiles = [canvas[:, y: y + 7, x: x + 11] for y, x in spots]
        ret = small_store.render_model(index=[0, 2], roi=rects, size=(7, 11), out=tiles, mean=MEAN, std=STD, dtype=dtype,
                                       mirror=[True, False], output_chroma_format=444, interpolation="bicubic", clamp=True)
        assert ret[0] is tiles[0] and ret[1] is tiles[1]
        mask = np.ones((3, 20, 40), dtype=bool)
        for (y, x), i, r, m in zip(spots, (0, 2), rects, (True, False)):
            q = _q(i, small_ref[(8, 444)][i], 8, 444, "rgb")
            _same(canvas[:, y: y + 7, x: x + 11], _finish(_resized((i, 8, 444, "rgb"), q, r, (7, 11), True), MEAN, STD, dtype, m),
                  (dtype, i))
            mask[:, y: y + 7, x: x + 11] = False
        assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), dtype


def test_resize_clamp_on_and_off(small, small_store, small_ref):
    """An upscale whose reference leaves [0, 1] on both sides: without the flag the values stay, with
    it they are clamped before the normalisation -- on both tails, from streams and store."""
    from ccmi import decode
    def leaves(rect, size):  # the REFERENCE leaves [0, 1] on both sides, for both streams
        rs = [_resized((i, 8, 444, "rgb"), _q(i, small_ref[(8, 444)][i], 8, 444, "rgb"), rect, size) for i in (0, 2)]
        return all(r.min() < 0 and r.max() > 1 for r in rs)
    found = [c for c in (((10, 4, 5, 4), (19, 23)), ((0, 0, 37, 21), (33, 58)), ((3, 5, 8, 8), (21, 37))) if leaves(*c)]
    assert found, "no candidate region overshoots on both sides"
    rect, size = found[0]
    for dtype in _dtypes():
        for clamp in (False, True):
            kw = dict(roi=rect, size=size, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444, interpolation="bicubic",
                      clamp=clamp)
            got = decode.decode_batch_model([small[0], small[2]], **kw)
            ren = _render(small_store, index=[0, 2], **kw)
            for j, i in enumerate((0, 2)):
                q = _q(i, small_ref[(8, 444)][i], 8, 444, "rgb")
                want = _finish(_resized((i, 8, 444, "rgb"), q, rect, size, clamp), MEAN, STD, dtype)
                _same(got[j], want, ("decode", clamp, dtype, i))
                _same(ren[j], want, ("render", clamp, dtype, i))


def test_bilinear_is_the_default_to_the_byte(small, small_store):
    import torch
    kw = dict(index=[0, 2], mean=MEAN, std=STD, dtype=torch.bfloat16, output_chroma_format=444)
    a = small_store.render_model(roi=(1, 1, 36, 20), size=(7, 5), **kw)
    b = small_store.render_model(roi=(1, 1, 36, 20), size=(7, 5), interpolation="bilinear", clamp=False, **kw)
    c = small_store.render_model(roi=(1, 1, 36, 20), size=(7, 5), interpolation="bicubic", **kw)
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(c))
    m = _mat(_rot(20, 1.2), (18, 10), (9, 11))
    a = small_store.render_model(affine=m.reshape(2, 3), size=(9, 11), **kw)
    b = small_store.render_model(affine=m.reshape(2, 3), size=(9, 11), interpolation="bilinear", **kw)
    c = small_store.render_model(affine=m.reshape(2, 3), size=(9, 11), interpolation="bicubic", **kw)
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(c))
    plan = dict(index=[0, 2], affine=m.reshape(2, 3), size=(9, 11), output_chroma_format=444)
    assert small_store.render_model_workspace_bytes(**plan) == \
        small_store.render_model_workspace_bytes(interpolation="bilinear", **plan)


# ------------------------------------------------------------------ the warp
def test_integer_translation_is_the_crop_and_flip_the_mirror(small, small_store, small_ref):
    """At fx = fy = 0 the outer coefficients are exactly 0: m = 1 0 x / 0 1 y equals
    render_model(roi=(x, y, w, h)) and m00 = -1 its mirror, bit for bit, clamp or not."""
    from ccmi import decode
    index = [0, 1, 2]
    for k, (x, y, w, h) in enumerate(((0, 0, 8, 8), (3, 5, 8, 8), (29, 13, 8, 8), (5, 0, 7, 21), (36, 20, 1, 1))):
        dtype = _dtypes()[k % 3]
        m = np.array([1, 0, x, 0, 1, y], np.float32).reshape(2, 3)
        f = np.array([-1, 0, x + w, 0, 1, y], np.float32).reshape(2, 3)
        kw = dict(mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444)
        plain = small_store.render_model(index=index, roi=(x, y, w, h), **kw)
        mirrored = small_store.render_model(index=index, roi=(x, y, w, h), mirror=True, **kw)
        warped = _render(small_store, index=index, affine=m, size=(h, w), interpolation="bicubic", clamp=bool(k & 1), **kw)
        flipped = _render(small_store, index=index, affine=f, size=(h, w), pad="edge", interpolation="bicubic", **kw)
        coded = decode.decode_batch_model(small, affine=[m] * 3, size=(h, w), pad="edge", interpolation="bicubic", **kw)
        for j in index:
            _same(warped[j], plain[j], ("store", dtype, j, x, y))
            _same(coded[j], plain[j], ("coded", dtype, j, x, y))
            _same(flipped[j], mirrored[j], ("flip", dtype, j, x, y))


# (matrix, size, pad, fill) on the 21 x 37 frames
WARPS = (
    (_mat(_rot(30), (0, 0), (12, 14)), (12, 14), "fill", FILL),           # about the top-left corner: taps outside
    (_mat(_rot(30), (0, 0), (12, 14)), (12, 14), "edge", 0.0),
    (_mat(_rot(-140, 0.7), (37, 21), (9, 13)), (9, 13), "fill", 0.0),      # about the bottom-right corner, zoomed out
    (_mat(_rot(-140, 0.7), (37, 21), (9, 13)), (9, 13), "edge", 0.0),
    (np.array([1, 0, 100, 0, 1, -50], np.float32), (4, 6), "fill", FILL),  # wholly outside the frame: all fill
    (np.array([1, 0, 100, 0, 1, -50], np.float32), (4, 6), "edge", 0.0),   # ... or the corner pixel
    (np.array([1, 0, 3, 0, 0.7, 1.3], np.float32), (11, 7), "fill", FILL),  # fx = 0 in every column, fy not
    (np.array([1.3, 0.2, -2.5, 0, 1, 4], np.float32), (9, 5), "edge", 0.0),  # fy = 0 in every row
    (_mat(_rot(7, 2.5), (18.5, 10.5), (21, 37)), (21, 37), "fill", FILL),   # zoomed in 2.5 x: the frame's middle
)


@pytest.mark.parametrize("case", range(len(WARPS)))
def test_warps_444(small, small_store, small_ref, case):
    from ccmi import decode
    m, size, pad, fill = WARPS[case]
    for k, dtype in enumerate(_dtypes()):
        bitdepth, colour = (8, 10, 8)[k], ("rgb", "asis")[k % 2]
        kw = dict(affine=m.reshape(2, 3), size=size, pad=pad, fill=fill, colour=colour, mean=MEAN, std=STD, dtype=dtype,
                  output_bitdepth=bitdepth, output_chroma_format=444, interpolation="bicubic")
        got = decode.decode_batch_model([small[0], small[2]], **kw)
        ren = _render(small_store, index=[0, 2], **kw)
        for j, i in enumerate((0, 2)):
            q = _q(i, small_ref[(bitdepth, 444)][i], bitdepth, 444, colour)
            want = _finish(_warped((i, bitdepth, colour), q, m, size, pad, fill), MEAN, STD, dtype)
            _same(got[j], want, ("decode", case, dtype, i))
            _same(ren[j], want, ("render", case, dtype, i))


def test_warp_420_mixed_matrices_one_group_mirror_nhwc_and_clamp(small, small_store, small_ref):
    """The 34 x 66 stream at its own 420 (even windows) and the 21 x 37 one at 444 in turn: four
    matrices in one call are one tail group; mirror flags, channels_last; the clamp acts where the
    reference leaves [0, 1] -- fill included (a fill of 1.5 is clamped to 1)."""
    from ccmi import decode
    size = (10, 9)
    for i, chroma, centre in ((1, 420, (33, 17)), (0, 444, (18, 10))):
        mats = [_mat(_rot(25, 1.6), centre, size), _mat(_rot(-70, 0.8), (2, 3), size), _mat(_rot(180, 2.2), centre, size),
                np.array([1, 0, 60, 0, 1, 30], np.float32)]
        flags = [False, True, True, False]
        q = _q(i, small_ref[(8, chroma)][i], 8, chroma, "rgb")
        fill = (1.5, -0.25, 0.5)
        over = False
        for k, dtype in enumerate(_dtypes()):
            clamp, pad = bool(k != 1), ("fill", "edge")[k == 2]
            kw = dict(index=[i] * 4, affine=np.stack(mats).reshape(4, 2, 3), size=size, pad=pad, fill=fill, mean=MEAN, std=STD,
                      dtype=dtype, mirror=flags, channels_last=bool(k & 1), output_chroma_format=chroma,
                      interpolation="bicubic", clamp=clamp)
            got = _render(small_store, **kw)
            assert decode.last_tail_groups() == (1, 0)
            for j, m in enumerate(mats):
                raw = _warped((i, 8, chroma), q, m, size, pad, fill, False)
                over = over or bool(raw.min() < 0 and raw.max() > 1)
                want = _finish(_warped((i, 8, chroma), q, m, size, pad, fill, clamp), MEAN, STD, dtype, flags[j])
                _same(got[j], want, (i, dtype, j))
        assert over


# ------------------------------------------------------------------ with the later stages
CONTRAST = [("brightness", 1.2), ("contrast", 1.6), ("saturation", 0.5)]
TONE = [("autocontrast", None), ("sharpness", 1.7), ("posterize", 4)]


def _staged(r, ops=None, tone=None, taps=None, th=None):
    """r' (after the mirror) through steps 3z, 3x and 3y, as tests/test_decode_tone_gpu.py composes them"""
    import torch
    x = torch.from_numpy(np.array(r))
    x = KR.apply(x, ops) if ops else x
    y = TR.apply(x, tone) if tone else x
    return FR.apply(y, taps, th) if (tone or FR.takes_stage(taps, th)) else y


@pytest.mark.parametrize("geometry", ("resize", "warp"))
def test_with_colour_ops_a_blur_and_tone_ops(small, small_store, small_ref, geometry):
    """One case each: colour_ops with a contrast op (the statistics pass of the cubic kernels), blur=
    and tone_ops= (the float32 identity-format instantiation stages the frame); clamp off, so values
    outside [0, 1] reach the first op, which clamps.  Window tail and per-frame tail, store and streams."""
    from ccmi import decode
    taps = decode.gaussian_taps(0.9, 5)
    size = (13, 11)
    m = _mat(_rot(33, 1.8), (17, 9), size)
    if geometry == "resize":
        geo = dict(roi=(10, 4, 5, 4), size=size)
    else:
        geo = dict(affine=m.reshape(2, 3), size=size, pad="fill", fill=FILL)
    stages = (dict(colour_ops=CONTRAST), dict(blur=taps, solarize=0.6), dict(tone_ops=TONE),
              dict(colour_ops=CONTRAST, tone_ops=TONE, blur=taps))
    for k, extra in enumerate(stages):
        dtype = _dtypes()[k % 3]
        kw = dict(mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444, interpolation="bicubic", **geo, **extra)
        got = decode.decode_batch_model([small[0], small[2]], **kw)
        ren = _render(small_store, index=[0, 2], **kw)
        for j, i in enumerate((0, 2)):
            q = _q(i, small_ref[(8, 444)][i], 8, 444, "rgb")
            r = _resized((i, 8, 444, "rgb"), q, geo["roi"], size) if geometry == "resize" else \
                _warped((i, 8, "rgb"), q, m, size, "fill", FILL)
            want = _finish(_staged(r, extra.get("colour_ops"), extra.get("tone_ops"), extra.get("blur"), extra.get("solarize")),
                           MEAN, STD, dtype)
            _same(got[j], want, ("decode", geometry, k, i))
            _same(ren[j], want, ("render", geometry, k, i))


# ------------------------------------------------------------------ Python errors
def test_python_errors(small, small_store):
    from ccmi import decode
    m = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    for bad in ("nearest", "lanczos", "BICUBIC", None):
        with pytest.raises(ValueError, match="interpolation"):
            decode.decode_batch_model(small[:1], size=(8, 8), interpolation=bad, output_chroma_format=444)
        with pytest.raises(ValueError, match="interpolation"):
            small_store.render_model(index=[0], affine=m, size=(8, 8), interpolation=bad, output_chroma_format=444)
        with pytest.raises(ValueError, match="interpolation"):
            small_store.render_model_workspace_bytes(index=[0], size=(8, 8), interpolation=bad, output_chroma_format=444)
        with pytest.raises(ValueError, match="interpolation"):
            small_store.warp_plan([0], m, (8, 8), interpolation=bad, output_chroma_format=444)
    for call in (lambda **kw: decode.decode_batch_model(small[:1], size=(8, 8), output_chroma_format=444, **kw),
                 lambda **kw: small_store.render_model(index=[0], affine=m, size=(8, 8), output_chroma_format=444, **kw),
                 lambda **kw: small_store.render_model_workspace_bytes(index=[0], size=(8, 8), output_chroma_format=444, **kw),
                 lambda **kw: small_store.warp_plan([0], m, (8, 8), output_chroma_format=444, **kw)):
        with pytest.raises(ValueError, match="clamp"):
            call(clamp=True)
        with pytest.raises(ValueError, match="clamp"):
            call(interpolation="bilinear", clamp=True)
    # warp_plan reports the cubic window: one tap more on every side the frame allows
    t = [[1, 0, 10], [0, 1, 6]]
    a = small_store.warp_plan([0], t, (4, 4), output_chroma_format=444)[0]["window"]
    b = small_store.warp_plan([0], t, (4, 4), output_chroma_format=444, interpolation="bicubic")[0]["window"]
    c = small_store.warp_plan([0], t, (4, 4), output_chroma_format=444, interpolation="bicubic", clamp=True)[0]["window"]
    assert a == (9, 5, 7, 7) and b == c == (8, 4, 9, 9)
