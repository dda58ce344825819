"""Tone ops in the decoder's output stage (ccmi_decode_batch_dev_tone / ccmi_latents_render_tone;
decode.decode_batch_model(tone_ops=...) and LatentStore.render_model(tone_ops=...)): per-frame lists of
brightness, saturation, contrast, matrix, solarize, posterize, autocontrast, equalize and sharpness on the
staged frame, after the geometry of all three paths and the colour ops, before blur / solarize and the
normalisation.

The reference is never the new code: render_model(float32, mean 0, std 1, the same mirror) of the same
frames WITHOUT tone ops and filter, put through tests/colour_ref.py where there are colour ops, through
tests/tone_ref.py (step 3x in numpy float32, pinned by tests/test_decode_tone_ref.py), through
tests/filter_ref.py, then scale, bias and .to(dtype).  Every comparison is BITWISE.

Streams: test_decode_filter_gpu.py's (class D 416 x 240, two generated 21 x 37 streams, one of them with a
generic synthesis and so on the per-frame tail, a Kodak stream).  The statistics and apply kernels give a
block 2048 consecutive pixels, the sharpness kernel a 32 x 32 tile: 33 x 65 (2145 pixels) and 5 x 129
straddle a block, a row of tiles and a tile width (four of them) by one.  A list holds at most 8 ops, so
"all ops in one list" is two lists of 8 that cover the nine between them."""
from pathlib import Path

import numpy as np
import pytest

import colour_ref as R
import filter_ref as F
import tone_ref as T
from test_decode_colour_gpu import FILL, PATHS, ROI, SIZE, _hue, _rot
from test_decode_fmt_gpu import MEAN, STD, _bits, _f32, _generate, _same, _sentinel_canvas

GOLDEN = Path(__file__).resolve().parent / "golden"

pytestmark = pytest.mark.gpu

M = np.array([[0.9, 0.2, 0.0, 0.01], [0.1, 0.8, 0.1, 0.0], [0.0, 0.3, 0.7, 0.02]], dtype=np.float32)
ALONE = [("brightness", 1.3), ("saturation", 0.4), ("contrast", 1.7), ("matrix", M), ("solarize", 0.5), ("posterize", 3),
         ("autocontrast", None), ("equalize", None), ("sharpness", 1.8)]
ALL_A = [("sharpness", 0.3), ("saturation", 1.4), ("equalize", None), ("posterize", 5), ("matrix", M), ("contrast", 0.6),
         ("autocontrast", None), ("solarize", 0.6)]
ALL_B = [("brightness", 0.8), ("autocontrast", None), ("sharpness", 1.9), ("solarize", 0.4), ("contrast", 1.4),
         ("posterize", 2), ("equalize", None), ("saturation", 0.7)]
TWICE = [("equalize", None), ("contrast", 1.5), ("brightness", 0.8), ("equalize", None), ("contrast", 0.5)]
SHARP_FIRST = [("sharpness", 1.7), ("brightness", 1.1), ("autocontrast", None)]
SHARP_LAST = [("posterize", 4), ("equalize", None), ("sharpness", 0.2)]
SHARP_TWICE = [("sharpness", 1.9), ("solarize", 0.7), ("sharpness", 0.0), ("contrast", 1.2)]


def _taps(r):
    from ccmi import decode
    return decode.gaussian_taps(0.3 * r + 0.4, 2 * r + 1)


@pytest.fixture(scope="module")
def data(gpu, ccmi_lib):
    """[class D 416 x 240 (420), 21 x 37, 21 x 37 with a generic synthesis, Kodak 512 x 768 (RGB)]"""
    d = sorted((GOLDEN / "cool").glob("D-*.cool"))[0].read_bytes()
    k = sorted((GOLDEN / "cool").rglob("kodim*.cool"))[0].read_bytes()
    return [d, _generate(21, 37, 7), _generate(21, 37, 11, generic=True), k]


@pytest.fixture(scope="module")
def store(data):
    from ccmi import decode
    st = decode.LatentStore(data)
    yield st
    st.close()


_BASE, _GROUPS = {}, {}


def _base(store, key, **kw):
    """The float32 render WITHOUT tone ops, filter and colour ops (mean 0, std 1) of a call's frames, on the
    CPU: computed once per key, shared and read-only; _GROUPS[key]: the tail groups that call ran."""
    from ccmi import decode
    if key not in _BASE:
        _BASE[key] = store.render_model(**kw).detach().cpu()
        _GROUPS[key] = decode.last_tail_groups()
    return _BASE[key]


def _want(base, tone, taps=None, th=None, ops=None, mean=None, std=None, dtype=None):
    import torch
    dtype = dtype or torch.float32
    x = R.apply(base, ops) if ops else base
    staged = bool(tone) or F.takes_stage(taps, th)
    y = T.apply(x, tone) if tone else x
    y = F.apply(y, taps, th) if staged else y
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    out = torch.stack([y[c] * _f32(1.0 / std[c]) + _f32(-mean[c] / std[c]) for c in range(3)])
    assert out.dtype == torch.float32
    return out.to(dtype)


def _check(got, base, tones, what, blur=None, sol=None, ops=None, **fmt):
    for j in range(len(tones)):
        _same(got[j], _want(base[j], tones[j], blur[j] if blur else None, sol[j] if sol else None,
                            ops[j] if ops else None, **fmt), (what, j))


@pytest.mark.parametrize("path", sorted(PATHS))
def test_each_op_alone_every_op_and_frames_without_ops_in_one_call(store, path):
    """Every op alone, the two lists that hold all nine, two equalizes and two contrasts in one list, and
    frames without ops in between, mirror on and off, in one call and one tail group."""
    from ccmi import decode
    tones = [[op] for op in ALONE[:5]] + [[]] + [[op] for op in ALONE[5:]] + [[], ALL_A, ALL_B, TWICE, []]
    n = len(tones)
    mirror = [bool(j % 3 == 1) for j in range(n)]
    kw = dict(index=[0] * n, mirror=mirror, **PATHS[path])
    base = _base(store, ("alone", path), **kw)
    got = store.render_model(tone_ops=tones, **kw)
    assert decode.last_tail_groups() == _GROUPS[("alone", path)] == (1, 0)
    _check(got, base, tones, path)
    for j in (5, 10, 14):  # not staged: the frame of the call without
        _same(got[j], base[j], (path, "no ops", j))
    for j in (0, 6, 7, 8, 9):
        assert not np.array_equal(_bits(got[j]), _bits(base[j])), (path, j)
    one = store.render_model(tone_ops=ALL_A, **kw)  # one list for every frame
    _same(one[3], _want(base[3], ALL_A), (path, "one list"))


def test_small_outputs(store, data):
    """1 x 1, 1 x 7 and 2 x 9 (sharpness leaves them, autocontrast meets hi == lo, equalize the identity LUT)
    and 3 x 3 (one interior pixel) on all three paths; stream 2 runs the per-frame tail."""
    from ccmi import decode
    index = [1, 2, 2, 1, 0, 2]
    tones = [[("sharpness", 1.8)], [("autocontrast", None)], [("equalize", None)], ALL_A, ALL_B, SHARP_TWICE]
    mirror = [False, True, False, True, False, True]
    for h, w in ((1, 1), (1, 7), (2, 9), (3, 3)):
        geos = {"fmt": dict(roi=(3, 5, w, h)), "size": dict(roi=(3, 5, 17, 11), size=(h, w)),
                "affine": dict(affine=_rot(-30, 1.25, (18.0, 10.0), (h, w)), size=(h, w), fill=FILL)}
        for name, geo in geos.items():
            kw = dict(index=index, output_chroma_format=444, mirror=mirror, **geo)
            base = _base(store, ("small", name, h, w), **kw)
            assert tuple(base.shape[-2:]) == (h, w)
            got = store.render_model(tone_ops=tones, **kw)
            groups = decode.last_tail_groups()
            assert groups == _GROUPS[("small", name, h, w)] and groups[1] == 3, (name, groups)
            _check(got, base, tones, (name, h, w))
            if h <= 2:  # sharpness alone: the frame itself
                _same(got[0], base[0] + 0.0, (name, h, w, "sharpness leaves it"))
            coded = decode.decode_batch_model([data[i] for i in index], tone_ops=tones,
                                              **{k: v for k, v in kw.items() if k != "index"})
            assert np.array_equal(_bits(coded), _bits(got)), (name, h, w)


@pytest.mark.parametrize("size", ((33, 65), (5, 129)))
def test_outputs_past_one_block_and_one_tile(store, size):
    """Sharpness first, last and twice, the lists of all ops and the repeated statistics, from the batched tail
    (a region of the class-D frame, and a resample) and the per-frame tail (the generic stream resampled
    up); float32 NCHW, bf16 NHWC, and fp16 views with odd strides into a sentinel canvas."""
    import torch
    h, w = size
    tones = [SHARP_FIRST, SHARP_LAST, SHARP_TWICE, ALL_A, ALL_B, TWICE]
    mirror = [False, True, True, False, True, False]
    for name, kw in (("fmt", dict(index=[0] * 6, roi=(100, 60, w, h), output_chroma_format=444)),
                     ("size", dict(index=[0, 2, 2, 0, 2, 0], roi=(4, 2, 30, 18), size=(h, w), output_chroma_format=444))):
        base = _base(store, ("tiles", name, size), mirror=mirror, **kw)
        assert tuple(base.shape[-2:]) == (h, w)
        got = store.render_model(tone_ops=tones, mirror=mirror, **kw)
        _check(got, base, tones, (name, "float32"))
        got = store.render_model(tone_ops=tones, mirror=mirror, mean=MEAN, std=STD, dtype=torch.bfloat16, channels_last=True,
                                 **kw)
        _check(got, base, tones, (name, "bf16 nhwc"), mean=MEAN, std=STD, dtype=torch.bfloat16)
        canvas, pat = _sentinel_canvas((3, 6 * (h + 1) + 1, w + 7), torch.float16)
        spots = [(1 + j * (h + 1), 1 + j % 4) for j in range(6)]
        tiles = [canvas[:, y: y + h, x: x + w] for y, x in spots]
        store.render_model(tone_ops=tones, mirror=mirror, mean=MEAN, std=STD, dtype=torch.float16, out=tiles, **kw)
        mask = np.ones(tuple(canvas.shape), dtype=bool)
        for j, (y, x) in enumerate(spots):
            _same(canvas[:, y: y + h, x: x + w], _want(base[j], tones[j], mean=MEAN, std=STD, dtype=torch.float16),
                  (name, "fp16 tile", j))
            mask[:, y: y + h, x: x + w] = False
        assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), name


def test_after_colour_ops_before_a_blur_with_a_mirror_and_a_visible_fill(store):
    """Colour ops (a contrast among them), then tone ops, then a blur of radius 1 and of radius 15 and a
    solarize; a warp near the frame's corner, whose fill is visible and counts in every statistic; frames
    that take the stage through the filter alone and frames that take nothing."""
    import torch
    from ccmi import decode
    cops = [[("contrast", 1.7), ("matrix", _hue(0.07))], [], [("saturation", 0.4), ("brightness", 1.3)], [], [], []]
    tones = [ALL_A, TWICE, SHARP_TWICE, [], [], [("autocontrast", None)]]
    blur = [_taps(1), _taps(15), None, _taps(3), None, None]
    sol = [None, 0.5, 0.25, None, None, None]
    mirror = [False, True, True, False, True, True]
    paths = dict(PATHS, corner=dict(affine=_rot(30, 0.5, (4.0, 6.0), SIZE), size=SIZE, fill=FILL))
    for path in sorted(paths):
        kw = dict(index=[0] * 6, mirror=mirror, **paths[path])
        base = _base(store, ("stack", path), **kw)
        if path == "corner":  # the fill is in the picture
            fill = torch.tensor(FILL).view(3, 1, 1)
            assert int((base[0] == fill).all(0).sum()) > 100
        for dtype, cl in ((torch.float32, False), (torch.bfloat16, True)):
            got = store.render_model(colour_ops=cops, tone_ops=tones, blur=blur, solarize=sol, mean=MEAN, std=STD,
                                     dtype=dtype, channels_last=cl, **kw)
            assert decode.last_tail_groups() == _GROUPS[("stack", path)] == (1, 0)
            _check(got, base, tones, (path, dtype), blur=blur, sol=sol, ops=cops, mean=MEAN, std=STD, dtype=dtype)
        # frames 3 and 4 are the _flt call's
        flt = store.render_model(colour_ops=cops, blur=blur, solarize=sol, mean=MEAN, std=STD, dtype=torch.bfloat16,
                                 channels_last=True, **kw)
        _same(got[3], flt[3], (path, "filter only"))
        _same(got[4], flt[4], (path, "nothing"))


def test_batch_invariance_alone_in_a_batch_reversed_and_twice(store, data):
    import torch
    from ccmi import decode
    lists = [ALL_A, TWICE, [], SHARP_TWICE, ALL_B, [("equalize", None)], SHARP_LAST]
    for path in sorted(PATHS):
        geo = PATHS[path]
        call = dict(mean=MEAN, std=STD, dtype=torch.bfloat16, **geo)
        batch = store.render_model(index=[0] * 7, tone_ops=lists, **call)
        again = store.render_model(index=[0] * 7, tone_ops=lists, **call)
        assert np.array_equal(_bits(batch), _bits(again)), path  # the accumulators are cleared
        back = store.render_model(index=[0] * 7, tone_ops=lists[::-1], **call)
        for j in range(7):
            _same(back[6 - j], batch[j], (path, "reversed", j))
            alone = store.render_model(index=[0], tone_ops=[lists[j]], **call)
            _same(alone[0], batch[j], (path, "alone", j))
        coded = decode.decode_batch_model(data[:1] * 7, tone_ops=lists, **call)
        assert np.array_equal(_bits(coded), _bits(batch)), path


def test_no_ops_is_the_flt_call(store):
    """tone_ops None, [] and all-empty lists: the bits and the workspace of the call without; frames without
    ops in a mixed batch keep the _flt call's bits, and the tail groups are the _flt call's."""
    import torch
    from ccmi import decode
    blur, sol = [_taps(2), None, None], [None, None, 0.5]
    for path in sorted(PATHS):
        kw = dict(index=[0] * 3, mean=MEAN, std=STD, dtype=torch.float16,
                  mirror=[False, True, False], **PATHS[path])
        ws = {k: v for k, v in kw.items() if k not in ("mean", "std", "dtype", "mirror")}
        for b, s in ((None, None), (blur, sol)):
            plain = store.render_model(blur=b, solarize=s, **kw)
            groups = decode.last_tail_groups()
            need = store.render_model_workspace_bytes(blur=b, solarize=s, **ws)
            for tone in (None, [], [[], [], []]):
                got = store.render_model(tone_ops=tone, blur=b, solarize=s, **kw)
                assert np.array_equal(_bits(got), _bits(plain)), (path, tone)
                assert store.render_model_workspace_bytes(tone_ops=tone, blur=b, solarize=s, **ws) == need
            mixed = store.render_model(tone_ops=[[], ALL_A, []], blur=b, solarize=s, **kw)
            assert decode.last_tail_groups() == groups, path
            _same(mixed[0], plain[0], (path, "count 0", 0))
            _same(mixed[2], plain[2], (path, "count 0", 2))
            assert not np.array_equal(_bits(mixed[1]), _bits(plain[1]))


def test_regions_of_different_sizes_in_one_batch(store):
    """size=: regions of three sizes, of two streams, share the launches; every frame its own list."""
    from ccmi import decode
    rois = [(100, 60, 64, 48), (0, 0, 21, 13), (200, 100, 31, 57), (2, 2, 8, 8)]
    index = [0, 1, 0, 2]
    tones = [ALL_B, SHARP_FIRST, TWICE, ALL_A]
    kw = dict(index=index, roi=rois, size=(19, 27), output_chroma_format=444)
    base = _base(store, "regions", **kw)
    got = store.render_model(tone_ops=tones, **kw)
    assert decode.last_tail_groups() == _GROUPS["regions"]
    _check(got, base, tones, "regions")


def test_a_workspace_of_exactly_the_planned_bytes(store):
    import torch
    from ccmi import CcmiError
    tones = [ALL_A, SHARP_TWICE, []]
    blur = [None, _taps(2), _taps(2)]
    for path in sorted(PATHS):
        geo = PATHS[path]
        oh, ow = (ROI[3], ROI[2]) if path == "fmt" else SIZE
        need = store.render_model_workspace_bytes(index=[0] * 3, tone_ops=tones, blur=blur, **geo)
        frame = -(-12 * oh * ow // 256) * 256
        assert need - store.render_model_workspace_bytes(index=[0] * 3, blur=blur, **geo) == \
            (frame + 256) + 3 * 512 + 2 * frame + 4 * 3328
        want = store.render_model(index=[0] * 3, tone_ops=tones, blur=blur, **geo)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        got = store.render_model(index=[0] * 3, tone_ops=tones, blur=blur, workspace=ws[:need], **geo)
        assert np.array_equal(_bits(got), _bits(want)), path
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), path  # nothing past the planned bytes is written
        dst = [torch.full((3,) + tuple(want.shape[-2:]), 7.0, device="cuda") for _ in range(3)]
        with pytest.raises(CcmiError, match="workspace of %d bytes, need %d" % (need - 1, need)):
            store.render_model(index=[0] * 3, tone_ops=tones, blur=blur, workspace=ws[: need - 1], out=dst, **geo)
        torch.cuda.synchronize()
        assert all(bool((d == 7.0).all()) for d in dst)


@pytest.mark.parametrize("drawer", ("rand_augment", "trivial_augment_wide"))
def test_the_drawers(store, drawer):
    """A seeded draw is reproducible, uses torchvision's ranges, is accepted by the plan and renders to the
    reference on its matrices and lists."""
    import torch
    from ccmi import decode
    n, size = 24, (24, 32)
    crop = decode.affine_matrix(size, (208.0, 120.0), 0.0, 0.25)  # a 96 x 128 window of the class-D frame
    draw = getattr(decode, drawer)
    kw = dict(num_ops=3, magnitude=9) if drawer == "rand_augment" else {}
    mats, tones = draw(n, generator=torch.Generator().manual_seed(3), size=size, base=crop, **kw)
    mats2, tones2 = draw(n, generator=torch.Generator().manual_seed(3), size=size, base=crop, **kw)
    assert np.array_equal(mats, mats2) and repr(tones) == repr(tones2)
    assert mats.shape == (n, 2, 3) and mats.dtype == np.float32 and len(tones) == n
    names = {op for t in tones for op, _ in t}
    assert names <= set(T.NAMES) and len(names) >= 4, names
    assert any(not np.allclose(m, np.asarray(crop)) for m in mats)  # some frame drew a geometric op
    for t in tones:
        for op, v in t:
            if op in ("brightness", "saturation", "contrast", "sharpness"):
                assert 0.0 <= v <= 1.99
            elif op == "posterize":
                assert v in (2, 3, 4, 5, 6, 7, 8)
            elif op == "solarize":
                assert 0.0 <= v <= 1.0
    call = dict(index=[0] * n, affine=mats, size=size, fill=FILL)
    assert store.render_model_workspace_bytes(tone_ops=tones, **call) >= store.render_model_workspace_bytes(**call)
    base = _base(store, ("drawer", drawer), **call)
    got = store.render_model(tone_ops=tones, mean=MEAN, std=STD, dtype=torch.bfloat16, **call)
    _check(got, base, tones, drawer, mean=MEAN, std=STD, dtype=torch.bfloat16)


def test_python_arguments_and_plan_errors(store):
    import torch
    from ccmi import CcmiError
    with pytest.raises(ValueError, match="one per frame"):
        store.render_model(index=[0, 0], roi=ROI, tone_ops=[[("equalize", None)]] * 3)
    with pytest.raises(ValueError, match="tone op 'hue'"):
        store.render_model(index=[0], roi=ROI, tone_ops=[("hue", 0.1)])
    with pytest.raises(ValueError, match="3 x 4"):
        store.render_model(index=[0], roi=ROI, tone_ops=[("matrix", [1.0, 2.0])])
    dst = [torch.full((3, 48, 64), 7.0, device="cuda")]
    for ops, what in (([("posterize", 9)], "posterize bits"), ([("sharpness", -1.0)], "factor"),
                      ([("solarize", float("nan"))], "threshold"), ([("equalize", None)] * 9, "9 tone ops")):
        with pytest.raises(CcmiError, match="frame 0.*" + what):
            store.render_model(index=[0], roi=ROI, out=dst, tone_ops=[ops])
    torch.cuda.synchronize()
    assert bool((dst[0] == 7.0).all())
