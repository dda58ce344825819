"""Coloured formatted output (ccmi_decode_batch_dev_col / ccmi_latents_render_col;
decode.decode_batch_model(colour_ops=...) and LatentStore.render_model(colour_ops=...)): per-frame
brightness, saturation, contrast and colour-matrix ops in the decoder's output stage, after the
geometry of all three paths (a region, size=, affine=) and before the normalisation.

The reference is never the new code: render_model(float32, mean 0, std 1) of the same frames
WITHOUT ops, which the formatted / resampled / warped tests pin bit for bit, put through
tests/colour_ref.py (step 3z restated with torch CPU float32 operations, pinned by
tests/test_decode_colour_ref.py), then scale, bias and .to(dtype).  Every comparison is BITWISE.

Streams: one committed class-D stream (416 x 240, 420: the YUV -> RGB matrix runs first), and the
formatted-output tests' generated 21 x 37 streams, one of them with a generic synthesis (the
per-frame tail, which runs the single-frame kernels).  Regions of 64 x 48, resized or warped to
32 x 24; an odd 17 x 11 region at 444; a 1 x 1 output."""
import itertools
import math
from pathlib import Path

import numpy as np
import pytest

import colour_ref as R
from test_decode_fmt_gpu import MEAN, STD, _bits, _f32, _generate, _same, _sentinel_canvas

GOLDEN = Path(__file__).resolve().parent / "golden"
FILL = (0.2, 0.5, 0.7)
ROI = (100, 60, 64, 48)  # x, y, w, h of the class-D frame
SIZE = (24, 32)

pytestmark = pytest.mark.gpu


def _hue(h):
    from ccmi import decode
    return decode.hue_matrix(h)


def _rot(deg, scale, centre, size):
    c, s = math.cos(math.radians(deg)) / scale, math.sin(math.radians(deg)) / scale
    a = np.array([[c, -s], [s, c]])
    t = np.asarray(centre, np.float64) - a @ np.array([size[1] / 2, size[0] / 2])
    return np.array([[a[0, 0], a[0, 1], t[0]], [a[1, 0], a[1, 1], t[1]]], np.float32)


# the three geometry paths on the class-D frame: what render_model takes besides the frames
PATHS = {
    "fmt": dict(roi=ROI),
    "size": dict(roi=ROI, size=SIZE),
    "affine": dict(affine=_rot(30, 0.5, (132.3, 84.6), SIZE), size=SIZE, fill=FILL),
}
FOUR = {"brightness": ("brightness", 1.3), "saturation": ("saturation", 0.4), "contrast": ("contrast", 1.7),
        "matrix": ("matrix", None)}  # the matrix: hue 0.07, filled in by _four()


def _four():
    ops = dict(FOUR)
    ops["matrix"] = ("matrix", _hue(0.07))
    return ops


@pytest.fixture(scope="module")
def data(gpu, ccmi_lib):
    """[class D 416 x 240 (420), 21 x 37, 21 x 37 with a generic synthesis]"""
    d = sorted((GOLDEN / "cool").glob("D-*.cool"))[0].read_bytes()
    return [d, _generate(21, 37, 7), _generate(21, 37, 11, generic=True)]


@pytest.fixture(scope="module")
def store(data):
    from ccmi import decode
    st = decode.LatentStore(data)
    yield st
    st.close()


_BASE = {}


def _base(store, key, **kw):
    """The float32 render WITHOUT ops (mean 0, std 1) of a call's frames, on the CPU: computed once
    per key, shared and read-only."""
    if key not in _BASE:
        t = store.render_model(**kw).detach().cpu()
        _BASE[key] = t
    return _BASE[key]


def _want(base, ops, mean=None, std=None, dtype=None):
    import torch
    dtype = dtype or torch.float32
    y = R.apply(base, ops)
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    out = torch.stack([y[c] * _f32(1.0 / std[c]) + _f32(-mean[c] / std[c]) for c in range(3)])
    assert out.dtype == torch.float32
    return out.to(dtype)


def _check(got, base, ops, what, **fmt):
    for j, o in enumerate(ops):
        _same(got[j], _want(base[j], o, **fmt), (what, j))


@pytest.mark.parametrize("path", sorted(PATHS))
def test_each_op_alone(store, path):
    """One op per frame, 13 frames in one call; frame 0 of the class-D stream."""
    from ccmi import decode
    ops = [[("brightness", 0.0)], [("brightness", 0.6)], [("brightness", 1.4)], [("saturation", 0.0)], [("saturation", 0.6)],
           [("saturation", 1.4)], [("contrast", 0.0)], [("contrast", 0.6)], [("contrast", 1.4)], [("matrix", _hue(-0.1))],
           [("matrix", decode.grey_matrix())], [("matrix", [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]])],
           [("matrix", [[-1, 0, 0, 1], [0, -1, 0, 1], [0, 0, -1, 1]])]]
    n = len(ops)
    kw = dict(index=[0] * n, **PATHS[path])
    base = _base(store, ("alone", path), **kw)
    got = store.render_model(colour_ops=ops, **kw)
    assert decode.last_tail_groups() == (1, 0)
    _check(got, base, ops, path)
    # one list for every frame
    one = store.render_model(colour_ops=ops[4], **kw)
    _same(one[3], got[4], (path, "one list"))


@pytest.mark.parametrize("path", sorted(PATHS))
def test_all_24_orders_and_frames_without_ops_in_one_call(store, path):
    from ccmi import decode
    four = _four()
    ops = [[four[k] for k in order] for order in itertools.permutations(sorted(four))]
    ops = ops[:7] + [[]] + ops[7:] + [[], []]
    assert len(ops) == 27
    kw = dict(index=[0] * 27, **PATHS[path])
    base = _base(store, ("orders", path), **kw)
    got = store.render_model(colour_ops=ops, **kw)
    assert decode.last_tail_groups() == (1, 0)
    _check(got, base, ops, path)
    for j in (7, 25, 26):  # no ops: the frame as it is without colour
        _same(got[j], base[j], (path, "no ops", j))
    assert len({_bits(got[j]).tobytes() for j in range(27)}) == 25


def test_clamps(store):
    """Factors 1.8 / 2.5 / 3.0 drive pixels to both ends of [0, 1]."""
    import torch
    ops = [[("brightness", 1.8)], [("saturation", 2.5)], [("contrast", 3.0)],
           [("brightness", 1.8), ("saturation", 2.5), ("contrast", 3.0)]]
    for path in sorted(PATHS):
        kw = dict(index=[0] * 4, **PATHS[path])
        base = _base(store, ("clamps", path), **kw)
        got = store.render_model(colour_ops=ops, **kw)
        wants = [_want(base[j], o) for j, o in enumerate(ops)]
        # on the reference: the call's elements sit at 0, at 1 and strictly between
        all_ = torch.stack(wants)
        assert bool((all_ == 0).any()) and bool((all_ == 1).any()) and bool(((all_ > 0) & (all_ < 1)).any()), path
        assert float(all_.min()) == 0.0 and float(all_.max()) == 1.0
        for j, want in enumerate(wants):
            _same(got[j], want, (path, j))


def test_the_mean_alone_in_a_batch_twice_and_mirrored(store, data):
    from ccmi import decode
    ops = [("saturation", 1.2), ("contrast", 0.45), ("brightness", 1.1)]
    for path in sorted(PATHS):
        geo = PATHS[path]
        others = [[("contrast", 2.0)], [], ops, [("brightness", 0.5), ("contrast", 1.9)], ops]
        mirror = [False, False, False, False, True]
        batch = store.render_model(index=[0] * 5, colour_ops=others, mirror=mirror, **geo)
        again = store.render_model(index=[0] * 5, colour_ops=others, mirror=mirror, **geo)
        assert np.array_equal(_bits(batch), _bits(again)), path
        alone = store.render_model(index=[0], colour_ops=[ops], **geo)
        _same(batch[2], alone[0], (path, "alone"))
        _same(batch[4], alone[0].flip(-1), (path, "mirrored"))
        base = _base(store, ("mean", path), index=[0], **geo)
        _same(alone[0], _want(base[0], ops), (path, "ref"))
        coded = decode.decode_batch_model(data[:1], colour_ops=[ops], **geo)
        _same(coded[0], alone[0], (path, "coded"))


def test_the_mean_counts_fill_pixels(store):
    """A warp whose output lies half outside the frame: the fill pixels count in the mean."""
    size = (24, 32)
    m = np.array([[1, 0, -16.0], [0, 1, 100.0]], np.float32)  # columns 0..15 sample x < 0
    ops = [("contrast", 0.3)]
    kw = dict(index=[0], affine=m, size=size, fill=FILL)
    base = _base(store, "fill", **kw)
    import torch
    assert bool((base[0][:, :, :15] == torch.tensor(FILL)[:, None, None]).all())
    got = store.render_model(colour_ops=ops, **kw)
    _same(got[0], _want(base[0], ops), "half fill")
    inside = _want(base[0][:, :, 16:].contiguous(), ops)
    assert not np.array_equal(_bits(got[0][:, :, 16:]), _bits(inside))  # the mean of the frame part alone differs


def test_the_sum_of_a_whole_frame_passes_2_to_the_32(store):
    """416 x 240 pixels at brightness 4 before the contrast op: S_j needs more than 32 bits."""
    import torch
    ops = [("brightness", 4.0), ("contrast", 0.5)]
    base = _base(store, "whole", index=[0])
    assert tuple(base.shape) == (1, 3, 240, 416)
    s = R.grey_sum(R.apply(base[0], ops[:1]))
    assert s > 2 ** 32, s
    got = store.render_model(index=[0], colour_ops=ops)
    _same(got[0], _want(base[0], ops), "whole frame")
    bf = store.render_model(index=[0], colour_ops=ops, mean=MEAN, std=STD, dtype=torch.bfloat16)
    _same(bf[0], _want(base[0], ops, MEAN, STD, torch.bfloat16), "whole frame, bf16")


def test_formats_layouts_and_a_view_into_a_canvas(store):
    """mean / std with bf16, fp16 and float32, NHWC, and tiles of a sentinel canvas: the
    restatement followed by steps 4-6; nothing outside the tiles changes."""
    import torch
    four = _four()
    ops = [[four["contrast"], four["matrix"]], [], [four["saturation"], four["brightness"], four["contrast"]]]
    for path in sorted(PATHS):
        kw = dict(index=[0] * 3, **PATHS[path])
        base = _base(store, ("formats", path), **kw)
        h, w = base.shape[-2:]
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            for cl in (False, True):
                got = store.render_model(colour_ops=ops, mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
                if cl:
                    assert tuple(got.stride()) == (h * w * 3, 1, w * 3, 3)
                _check(got, base, ops, (path, dtype, cl), mean=MEAN, std=STD, dtype=dtype)
            canvas, pat = _sentinel_canvas((3, 2 * h + 9, 2 * w + 7), dtype)
            spots = ((1, 3), (h + 4, w + 5), (h + 6, 2))
            tiles = [canvas[:, y: y + h, x: x + w] for y, x in spots]
            ret = store.render_model(colour_ops=ops, out=tiles, mean=MEAN, std=STD, dtype=dtype, **kw)
            assert ret[0] is tiles[0]
            mask = np.ones(tuple(canvas.shape), dtype=bool)
            for j, (y, x) in enumerate(spots):
                _same(canvas[:, y: y + h, x: x + w], _want(base[j], ops[j], MEAN, STD, dtype), (path, dtype, "tile", j))
                mask[:, y: y + h, x: x + w] = False
            assert (_bits(canvas)[mask] == np.array(pat).astype(_bits(canvas).dtype)).all(), (path, dtype)


def test_odd_444_region_a_1x1_output_and_the_per_frame_tail(store, data):
    """17 x 11 at 444 from the generated streams (stream 2 runs the per-frame tail: the
    single-frame kernels), and 1 x 1 outputs on all three paths."""
    from ccmi import decode
    four = _four()
    ops = [[four[k] for k in o] for o in (("contrast", "matrix", "brightness", "saturation"),
                                          ("matrix", "saturation"), ("brightness", "contrast"), ())]
    index = [1, 2, 2, 1]
    geos = {"fmt": dict(roi=(3, 5, 17, 11)), "size": dict(roi=(3, 5, 17, 11), size=(7, 5)),
            "affine": dict(affine=_rot(-30, 1.25, (30.0, 12.0), (7, 5)), size=(7, 5), fill=FILL, pad="fill"),
            "fmt1": dict(roi=(36, 20, 1, 1)), "size1": dict(roi=(3, 5, 17, 11), size=(1, 1)),
            "affine1": dict(affine=_rot(45, 0.5, (10.0, 8.0), (1, 1)), size=(1, 1), pad="edge")}
    for name, geo in geos.items():
        kw = dict(index=index, output_chroma_format=444, **geo)
        base = _base(store, ("odd", name), **kw)
        got = store.render_model(colour_ops=ops, **kw)
        assert decode.last_tail_groups() == (1, 2), name
        _check(got, base, ops, name)
        coded = decode.decode_batch_model([data[i] for i in index], colour_ops=ops, output_chroma_format=444, **geo)
        assert np.array_equal(_bits(coded), _bits(got)), name
    # 'asis' on the YUV stream: the ops act on the channels whatever they are
    kw = dict(index=[0, 0], roi=ROI, colour="asis")
    base = _base(store, "asis", **kw)
    got = store.render_model(colour_ops=ops[:2], **kw)
    _check(got, base, ops[:2], "asis")


def test_coded_streams_an_int16_store_and_its_compaction_agree(data):
    import torch
    from ccmi import decode
    four = _four()
    ops = [[four["brightness"], four["contrast"]], [four["contrast"], four["saturation"], four["matrix"]]]
    st16 = decode.LatentStore(data[:1], dtype=torch.int16)
    seg = st16.compact()
    try:
        for path in sorted(PATHS):
            kw = dict(colour_ops=ops, mean=MEAN, std=STD, dtype=torch.bfloat16, **PATHS[path])
            coded = decode.decode_batch_model(data[:1] * 2, **kw)
            a = st16.render_model(index=[0, 0], **kw)
            b = seg.render_model(index=[0, 0], **kw)
            assert np.array_equal(_bits(coded), _bits(a)) and np.array_equal(_bits(a), _bits(b)), path
    finally:
        seg.close()
        st16.close()


def test_none_and_empty_ops_are_the_call_without(store, data):
    import torch
    from ccmi import decode
    for path in sorted(PATHS):
        kw = dict(index=[0, 0], mean=MEAN, std=STD, dtype=torch.float16, mirror=[False, True], **PATHS[path])
        plain = store.render_model(**kw)
        need = store.render_model_workspace_bytes(index=[0, 0], **PATHS[path])
        for ops in (None, [], [[], []]):
            got = store.render_model(colour_ops=ops, **kw)
            assert np.array_equal(_bits(got), _bits(plain)), (path, ops)
            assert store.render_model_workspace_bytes(index=[0, 0], colour_ops=ops, **PATHS[path]) == need
        coded = decode.decode_batch_model(data[:1] * 2, colour_ops=[], **{k: v for k, v in kw.items() if k != "index"})
        assert np.array_equal(_bits(coded), _bits(plain)), path


def test_a_workspace_of_exactly_the_planned_bytes(store):
    import torch
    from ccmi import CcmiError
    ops = [[("contrast", 1.2)], [("brightness", 0.9)]]
    for path in sorted(PATHS):
        geo = PATHS[path]
        need = store.render_model_workspace_bytes(index=[0, 0], colour_ops=ops, **geo)
        assert need > store.render_model_workspace_bytes(index=[0, 0], **geo)
        want = store.render_model(index=[0, 0], colour_ops=ops, **geo)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        got = store.render_model(index=[0, 0], colour_ops=ops, workspace=ws[:need], **geo)
        assert np.array_equal(_bits(got), _bits(want)), path
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), path  # nothing past the planned bytes is written
        dst = [torch.full((3,) + tuple(want.shape[-2:]), 7.0, device="cuda") for _ in range(2)]
        with pytest.raises(CcmiError, match="workspace of %d bytes, need %d" % (need - 1, need)) as e:
            store.render_model(index=[0, 0], colour_ops=ops, workspace=ws[: need - 1], out=dst, **geo)
        assert e.value.code == 1  # CCMI_ERR_ARG
        torch.cuda.synchronize()
        assert bool((dst[0] == 7.0).all()) and bool((dst[1] == 7.0).all())


def test_python_arguments_and_plan_errors(store):
    import torch
    from ccmi import CcmiError
    with pytest.raises(ValueError, match="one per frame"):
        store.render_model(index=[0, 0], roi=ROI, colour_ops=[[("brightness", 1.0)]] * 3)
    with pytest.raises(ValueError, match="colour op"):
        store.render_model(index=[0], roi=ROI, colour_ops=[("gamma", 1.0)])
    with pytest.raises(ValueError, match="3 x 4"):
        store.render_model(index=[0], roi=ROI, colour_ops=[("matrix", [1, 0, 0])])
    dst = [torch.full((3, 48, 64), 7.0, device="cuda")]
    for ops, what in (([("contrast", 1.0), ("contrast", 1.0)], "contrast"), ([("brightness", -1.0)], "factor"),
                      ([("saturation", 1.0)] * 9, "9 colour ops"), ([(5, 1.0)], "unknown op")):
        with pytest.raises(CcmiError, match="frame 0.*" + what):
            store.render_model(index=[0], roi=ROI, colour_ops=ops, out=dst)
    torch.cuda.synchronize()
    assert bool((dst[0] == 7.0).all())
