"""Filtered formatted output (ccmi_decode_batch_dev_flt / ccmi_latents_render_flt;
decode.decode_batch_model(blur=..., solarize=...) and LatentStore.render_model(blur=..., solarize=...)):
a per-frame separable blur with reflecting borders and a per-frame solarize in the decoder's output
stage, after the geometry of all three paths (a region, size=, affine=) and the colour ops, before the
normalisation.

The reference is never the new code: render_model(float32, mean 0, std 1, the same mirror) of the same
frames WITHOUT a filter, which the formatted / resampled / warped tests pin bit for bit, put through
tests/colour_ref.py where there are ops and through tests/filter_ref.py (steps 3y-0 .. 3y-2 restated with
torch CPU float32 operations, pinned by tests/test_decode_filter_ref.py), then scale, bias and
.to(dtype).  Every comparison is BITWISE.

Streams: one committed class-D stream (416 x 240, 420), a committed Kodak stream (RGB), and the
formatted-output tests' generated 21 x 37 streams, one of them with a generic synthesis (the per-frame
tail, which runs the single-frame kernel).  The filter kernel's tile is 32 rows x 16 groups of 4 pixels
(64 columns): the 75 x 141 outputs have a first, an interior and a partial last tile on both axes."""
from pathlib import Path

import numpy as np
import pytest

import colour_ref as R
import filter_ref as F
from test_decode_colour_gpu import FILL, PATHS, ROI, SIZE, _hue, _rot
from test_decode_fmt_gpu import MEAN, STD, _bits, _f32, _generate, _same, _sentinel_canvas

GOLDEN = Path(__file__).resolve().parent / "golden"

pytestmark = pytest.mark.gpu


def _taps(r, sigma=None):
    from ccmi import decode
    return decode.gaussian_taps(sigma or 0.3 * r + 0.4, 2 * r + 1)


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
    """The float32 render WITHOUT a filter and without ops (mean 0, std 1) of a call's frames, on the
    CPU: computed once per key, shared and read-only; _GROUPS[key]: the tail groups that call ran."""
    from ccmi import decode
    if key not in _BASE:
        _BASE[key] = store.render_model(**kw).detach().cpu()
        _GROUPS[key] = decode.last_tail_groups()
    return _BASE[key]


def _want(base, taps, th, ops=None, mean=None, std=None, dtype=None):
    import torch
    dtype = dtype or torch.float32
    x = R.apply(base, ops) if ops else base
    y = F.apply(x, taps, th) if F.takes_stage(taps, th) else x
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    out = torch.stack([y[c] * _f32(1.0 / std[c]) + _f32(-mean[c] / std[c]) for c in range(3)])
    assert out.dtype == torch.float32
    return out.to(dtype)


def _check(got, base, blur, sol, what, ops=None, **fmt):
    for j in range(len(blur)):
        _same(got[j], _want(base[j], blur[j], sol[j], ops[j] if ops else None, **fmt), (what, j))


@pytest.mark.parametrize("path", sorted(PATHS))
def test_radii_0_to_15_and_frames_without_a_filter_in_one_call(store, path):
    """Solarize alone (radius 0), radii 1 .. 15 and three frames that do not take the stage, mirror on and
    off, in one call and one tail group; the frames that do not take it keep the bits of the call without."""
    from ccmi import decode
    blur = [None] + [_taps(r) for r in range(1, 16)] + [None, None, _taps(1)[:1]]
    sol = [0.5] + [None] * 7 + [0.25] + [None] * 7 + [None, 2.0, None]
    n = len(blur)
    mirror = [bool(j % 3 == 1) for j in range(n)]
    kw = dict(index=[0] * n, mirror=mirror, **PATHS[path])
    base = _base(store, ("radii", path), **kw)
    got = store.render_model(blur=blur, solarize=sol, **kw)
    assert decode.last_tail_groups() == _GROUPS[("radii", path)] == (1, 0)
    _check(got, base, blur, sol, path)
    for j in (16, 17, 18):  # not staged: the frame of the call without a filter
        _same(got[j], base[j], (path, "no filter", j))
    assert not np.array_equal(_bits(got[1]), _bits(base[1]))
    # one entry and one threshold for every frame
    one = store.render_model(blur=blur[5], solarize=0.25, **kw)
    _same(one[8], _want(base[8], blur[5], 0.25), (path, "one entry"))


def test_small_outputs_fold_the_reflection_more_than_once(store, data):
    """1 x 1, 2 x 3 and 5 x 7 outputs with r = 11 and r = 15 on all three paths; stream 2 runs the
    per-frame tail (the single-frame kernel)."""
    from ccmi import decode
    index = [1, 2, 2, 1, 0]
    blur = [_taps(11), _taps(11), _taps(15), _taps(15), _taps(15, 5.0)]
    sol = [None, 0.5, None, None, None]
    for h, w in ((1, 1), (2, 3), (5, 7)):
        geos = {"fmt": dict(roi=(3, 5, w, h)), "size": dict(roi=(3, 5, 17, 11), size=(h, w)),
                "affine": dict(affine=_rot(-30, 1.25, (18.0, 10.0), (h, w)), size=(h, w), fill=FILL)}
        for name, geo in geos.items():
            kw = dict(index=index, output_chroma_format=444, mirror=[False, True, False, True, False], **geo)
            base = _base(store, ("small", name, h, w), **kw)
            assert tuple(base.shape[-2:]) == (h, w)
            got = store.render_model(blur=blur, solarize=sol, **kw)
            groups = decode.last_tail_groups()
            assert groups == _GROUPS[("small", name, h, w)] and groups[1] == 2, (name, groups)
            _check(got, base, blur, sol, (name, h, w))
            coded = decode.decode_batch_model([data[i] for i in index], blur=blur, solarize=sol,
                                              **{k: v for k, v in kw.items() if k != "index"})
            assert np.array_equal(_bits(coded), _bits(got)), (name, h, w)


def test_an_output_of_three_tiles_each_way(store):
    """75 x 141: tiles of 32 rows (32, 32, 11) and of 16 groups (36 groups: 16, 16, 4), from the batched
    tail (a region of the class-D frame, and its resample) and from the per-frame tail (the generic
    21 x 37 stream resampled up); bf16 NCHW, fp16 NHWC, and float32 views into a canvas whose rows start
    1, 2 and 3 elements off a 16-byte boundary (the groups' lead-in)."""
    import torch
    blur, sol, mirror = [_taps(15), _taps(3), None], [None, 0.5, 0.5], [False, True, True]
    for name, kw in (("fmt", dict(index=[0] * 3, roi=(100, 60, 141, 75), output_chroma_format=444)),
                     ("size", dict(index=[0, 2, 2], roi=(4, 2, 30, 18), size=(75, 141), output_chroma_format=444))):
        base = _base(store, ("tiles", name), mirror=mirror, **kw)
        assert tuple(base.shape[-2:]) == (75, 141)
        for dtype, cl in ((torch.bfloat16, False), (torch.float16, True)):
            got = store.render_model(blur=blur, solarize=sol, mirror=mirror, mean=MEAN, std=STD, dtype=dtype,
                                     channels_last=cl, **kw)
            _check(got, base, blur, sol, (name, dtype), mean=MEAN, std=STD, dtype=dtype)
        canvas, pat = _sentinel_canvas((3, 3 * 75 + 9, 141 + 8), torch.float32)
        spots = ((1, 1), (75 + 3, 2), (2 * 75 + 5, 3))
        tiles = [canvas[:, y: y + 75, x: x + 141] for y, x in spots]
        store.render_model(blur=blur, solarize=sol, mirror=mirror, out=tiles, **kw)
        mask = np.ones(tuple(canvas.shape), dtype=bool)
        for j, (y, x) in enumerate(spots):
            _same(canvas[:, y: y + 75, x: x + 141], _want(base[j], blur[j], sol[j]), (name, "tile", j))
            mask[:, y: y + 75, x: x + 141] = False
        assert (_bits(canvas)[mask] == pat).all(), name


def test_colour_ops_formats_layouts_and_a_view_into_a_canvas(store):
    """Colour ops (contrast among them) followed by the filter; solarize after a blur with thresholds 0, 0.5, 1
    and 2; mean / std with bf16, fp16 and float32, NHWC, and tiles of a sentinel canvas: nothing outside
    the tiles changes."""
    import torch
    from ccmi import decode
    ops = [[("contrast", 1.7), ("matrix", _hue(0.07))], [], [("saturation", 0.4), ("brightness", 1.3), ("contrast", 0.6)], []]
    blur, sol = [_taps(5), _taps(2), _taps(7), _taps(4)], [0.0, 0.5, 1.0, 2.0]
    mirror = [False, True, True, False]
    for path in sorted(PATHS):
        kw = dict(index=[0] * 4, mirror=mirror, **PATHS[path])
        base = _base(store, ("formats", path), **kw)
        h, w = base.shape[-2:]
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            for cl in (False, True):
                got = store.render_model(colour_ops=ops, blur=blur, solarize=sol, mean=MEAN, std=STD, dtype=dtype,
                                         channels_last=cl, **kw)
                assert decode.last_tail_groups() == (1, 0)
                if cl:
                    assert tuple(got.stride()) == (h * w * 3, 1, w * 3, 3)
                _check(got, base, blur, sol, (path, dtype, cl), ops=ops, mean=MEAN, std=STD, dtype=dtype)
            canvas, pat = _sentinel_canvas((3, 2 * h + 9, 2 * w + 7), dtype)
            spots = ((1, 3), (h + 4, w + 5), (h + 6, 2), (2, w + 6))
            tiles = [canvas[:, y: y + h, x: x + w] for y, x in spots]
            ret = store.render_model(colour_ops=ops, blur=blur, solarize=sol, out=tiles, mean=MEAN, std=STD, dtype=dtype, **kw)
            assert ret[0] is tiles[0]
            mask = np.ones(tuple(canvas.shape), dtype=bool)
            for j, (y, x) in enumerate(spots):
                _same(canvas[:, y: y + h, x: x + w], _want(base[j], blur[j], sol[j], ops[j], MEAN, STD, dtype),
                      (path, dtype, "tile", j))
                mask[:, y: y + h, x: x + w] = False
            assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), (path, dtype)


def test_solarize_alone_a_420_and_an_rgb_stream_and_asis(store, data):
    """Solarize without any blur in the call (taps NULL), on the 420 class-D stream, the RGB Kodak stream
    and the generated streams, thresholds 0, 0.5, 1 and 2; and a blur on the stream's own planes ('asis')."""
    from ccmi import decode
    index, sol = [0, 3, 1, 2, 3], [0.5, 0.5, 0.0, 1.0, 2.0]
    kw = dict(index=index, roi=(2, 4, 32, 16))
    base = _base(store, "solarize", **kw)
    got = store.render_model(solarize=sol, **kw)
    groups = decode.last_tail_groups()
    assert groups == _GROUPS["solarize"] and groups[1] == 1, groups
    _check(got, base, [None] * 5, sol, "solarize")
    _same(got[4], base[4], "threshold 2: off")
    coded = decode.decode_batch_model([data[i] for i in index], roi=kw["roi"], solarize=sol)
    assert np.array_equal(_bits(coded), _bits(got))
    blur = [_taps(6), _taps(9)]
    for colour in ("rgb", "asis"):
        kw = dict(index=[0, 3], roi=(2, 4, 32, 16), colour=colour)
        base = _base(store, ("asis", colour), **kw)
        got = store.render_model(blur=blur, **kw)
        _check(got, base, blur, [None, None], colour)


def test_a_frame_alone_in_a_batch_twice_and_from_coded_streams(store, data):
    import torch
    from ccmi import decode
    ops = [("saturation", 1.2), ("contrast", 0.45)]
    for path in sorted(PATHS):
        geo = PATHS[path]
        blur = [_taps(3), None, _taps(9), _taps(9), None]
        sol = [None, None, 0.5, 0.5, 0.25]
        cops = [[("contrast", 2.0)], [], ops, ops, []]
        mirror = [False, False, False, True, False]
        call = dict(blur=blur, solarize=sol, colour_ops=cops, mirror=mirror, mean=MEAN, std=STD, dtype=torch.bfloat16, **geo)
        batch = store.render_model(index=[0] * 5, **call)
        again = store.render_model(index=[0] * 5, **call)
        assert np.array_equal(_bits(batch), _bits(again)), path
        alone = store.render_model(index=[0], blur=[blur[2]], solarize=[sol[2]], colour_ops=[ops], mean=MEAN, std=STD,
                                   dtype=torch.bfloat16, **geo)
        _same(batch[2], alone[0], (path, "alone"))
        coded = decode.decode_batch_model(data[:1] * 5, **call)
        assert np.array_equal(_bits(coded), _bits(batch)), path
        # the frames that do not take the stage: the call without a filter, in the call's format
        plain = store.render_model(index=[0] * 5, colour_ops=cops, mirror=mirror, mean=MEAN, std=STD, dtype=torch.bfloat16,
                                   **geo)
        groups = decode.last_tail_groups()
        _same(batch[1], plain[1], (path, "not staged"))
        store.render_model(index=[0] * 5, **call)
        assert decode.last_tail_groups() == groups == (1, 0)


def test_no_filter_is_the_call_without(store, data):
    import torch
    from ccmi import decode
    for path in sorted(PATHS):
        kw = dict(index=[0, 0], mean=MEAN, std=STD, dtype=torch.float16, mirror=[False, True], **PATHS[path])
        plain = store.render_model(**kw)
        need = store.render_model_workspace_bytes(index=[0, 0], **PATHS[path])
        for blur, sol in ((None, None), ([None, None], None), (None, [None, 2.0]), ([_taps(1)[:1], None], [1.5, None])):
            got = store.render_model(blur=blur, solarize=sol, **kw)
            assert np.array_equal(_bits(got), _bits(plain)), (path, blur, sol)
            assert store.render_model_workspace_bytes(index=[0, 0], blur=blur, solarize=sol, **PATHS[path]) == need


def test_a_workspace_of_exactly_the_planned_bytes(store):
    import torch
    from ccmi import CcmiError
    blur, sol = [_taps(4), None], [None, 0.5]
    ops = [[("contrast", 1.2)], [("brightness", 0.9)]]
    for path in sorted(PATHS):
        geo = PATHS[path]
        need = store.render_model_workspace_bytes(index=[0, 0], colour_ops=ops, blur=blur, solarize=sol, **geo)
        oh, ow = (ROI[3], ROI[2]) if path == "fmt" else SIZE
        assert need - store.render_model_workspace_bytes(index=[0, 0], colour_ops=ops, **geo) == \
            2 * (-(-12 * oh * ow // 256) * 256 + 256)
        want = store.render_model(index=[0, 0], colour_ops=ops, blur=blur, solarize=sol, **geo)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        got = store.render_model(index=[0, 0], colour_ops=ops, blur=blur, solarize=sol, workspace=ws[:need], **geo)
        assert np.array_equal(_bits(got), _bits(want)), path
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), path  # nothing past the planned bytes is written
        dst = [torch.full((3,) + tuple(want.shape[-2:]), 7.0, device="cuda") for _ in range(2)]
        with pytest.raises(CcmiError, match="workspace of %d bytes, need %d" % (need - 1, need)) as e:
            store.render_model(index=[0, 0], colour_ops=ops, blur=blur, solarize=sol, workspace=ws[: need - 1], out=dst, **geo)
        assert e.value.code == 1  # CCMI_ERR_ARG
        torch.cuda.synchronize()
        assert bool((dst[0] == 7.0).all()) and bool((dst[1] == 7.0).all())


def test_python_arguments_and_plan_errors(store):
    import torch
    from ccmi import CcmiError
    with pytest.raises(ValueError, match="one per frame"):
        store.render_model(index=[0, 0], roi=ROI, blur=[_taps(2)] * 3)
    with pytest.raises(ValueError, match="one per frame"):
        store.render_model(index=[0, 0], roi=ROI, solarize=[0.5] * 3)
    with pytest.raises(ValueError, match="half taps"):
        store.render_model(index=[0], roi=ROI, blur=np.zeros(17, dtype=np.float32))
    dst = [torch.full((3, 48, 64), 7.0, device="cuda")]
    nan = np.array([0.5, float("nan")], dtype=np.float32)
    for kw, what in ((dict(blur=[nan]), "tap 1"), (dict(solarize=[float("nan")]), "threshold"),
                     (dict(blur=[np.array([0.5, float("inf")], dtype=np.float32)], solarize=[0.5]), "tap 1")):
        with pytest.raises(CcmiError, match="frame 0.*" + what):
            store.render_model(index=[0], roi=ROI, out=dst, **kw)
    torch.cuda.synchronize()
    assert bool((dst[0] == 7.0).all())
