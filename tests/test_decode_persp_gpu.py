"""The perspective warp of the decoder's output stage (CCMI_WARP_PROJECTIVE; perspective= of
decode.decode_batch_model and LatentStore.render_model) on the GPU.

The reference is never the new code: the bytes of decode.decode_batch, split into planes, steps 1-3 of
the ccmi_tensor_fmt contract over the WHOLE frame restated with torch CPU float32 operations
(tests/test_decode_warp_gpu.py's _q), step 3a' and the taps in numpy float32 one rounded operation at a
time (tests/persp_ref.py, pinned by tests/test_decode_persp_ref.py), then scale, bias and .to(dtype).
Every comparison is BITWISE for float32, float16 and bfloat16.  The reference samples the whole decoded
frame, so a window that is too small shows as wrong values.  Where the later stages take part
(colour_ops, tone_ops, blur) the reference is the affine= call of the same library with the same
matrix, whose own tests pin it: rows 0 0 1 must reproduce it element for element.

Streams: the first committed class-D stream (416 x 240, 420) and the first Kodak stream (RGB).  Output
sizes 1 x 1, 5 x 3, 37 x 29 and 64 x 48 (width x height): no multiple of the four pixels a thread writes
but the last."""
from pathlib import Path

import numpy as np
import pytest

import persp_ref as PR
from test_decode_cubic_gpu import _finish
from test_decode_fmt_gpu import MEAN, STD, _bits, _generate, _planes, _same
from test_decode_persp_abi import _first_with_rank
from test_decode_warp_gpu import _mat, _q, _rot

GOLDEN = Path(__file__).resolve().parent / "golden"
FILL = (0.2, 0.5, 0.7)
SIZES = ((1, 1), (3, 5), (29, 37), (48, 64))  # (out_h, out_w)
MODES = (("bilinear", False, 0), ("bicubic", False, PR.WARP_CUBIC), ("bicubic", True, PR.WARP_CUBIC | PR.WARP_CLAMP))

pytestmark = pytest.mark.gpu


def _dtypes():
    import torch
    return (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def frames(gpu, ccmi_lib):
    """[(stream bytes, H, W, q over the whole frame)] of the class-D and the Kodak stream; q is steps 1-3
    at the stream's own sample format, RGB."""
    from ccmi import decode
    d = sorted((GOLDEN / "cool").glob("D-*.cool"))[0].read_bytes()
    planes = _planes(decode.decode_batch([d], as_yuv=True)[0], 240, 416, 8, 420)
    out = [(d, 240, 416, _q("persp-D", planes, 8, 420, "rgb"))]
    k = sorted((GOLDEN / "cool").rglob("kodim*.cool"))[0].read_bytes()
    geom, _ = decode.decode_batch_geometry([k])
    h, w = geom[0]["height"], geom[0]["width"]
    ppm, = decode.decode_batch([k], as_yuv=False)
    hdr = b"P6\n%d %d\n255\n" % (w, h)
    kplanes = list(np.frombuffer(ppm[len(hdr):], dtype="u1").reshape(h, w, 3).transpose(2, 0, 1))
    out.append((k, h, w, _q("persp-kodak", kplanes, 8, 444, "rgb", yuv=False)))
    return out


@pytest.fixture(scope="module")
def stores(frames):
    """The int16 store of both streams and its compacted form."""
    from ccmi import decode
    st = decode.LatentStore([f[0] for f in frames])
    cp = st.compact()
    yield st, cp
    cp.close()
    st.close()


_REF = {}


def _ref(i, q, m, size, pad_word, fill=FILL):
    """r' of frame i for matrix m: [3, out_h, out_w] float32, computed once and read-only."""
    k = (i, tuple(np.asarray(m, np.float32).reshape(9).tolist()), size, pad_word, tuple(np.atleast_1d(fill).tolist()))
    if k not in _REF:
        r = PR.render(q, m, size[0], size[1], pad_word | PR.WARP_PROJECTIVE, fill)
        r.setflags(write=False)
        _REF[k] = r
    return _REF[k]


def _mats(frames, index, size, seed):
    """One accepted random homography per output frame, for its stream's frame size."""
    rng = np.random.default_rng(seed)
    return np.stack([PR.accepted_homographies(rng, 1, frames[i][1], frames[i][2], size[0], size[1], scales=(1.0, 0.01, 37.0))[0]
                     for i in index]).reshape(-1, 3, 3)


# ------------------------------------------------------------------ bitwise against the reference
@pytest.mark.parametrize("size", SIZES)
def test_bitwise_against_the_reference(frames, stores, size):
    """Both interpolations, clamp on and off, fill and edge, mirror flags within the call, NCHW and NHWC,
    three element types; from the streams, the int16 store and the compacted store."""
    from ccmi import decode
    index = [0, 1, 0, 1]
    flags = [False, True, True, False]
    mats = _mats(frames, index, size, 100 + size[0])
    data = [frames[i][0] for i in index]
    n = 0
    for dtype in _dtypes():
        for interpolation, clamp, word in MODES:
            for pad in ("fill", "edge"):
                kw = dict(perspective=mats, size=size, pad=pad, fill=FILL, mean=MEAN, std=STD, dtype=dtype, mirror=flags,
                          interpolation=interpolation, clamp=clamp)
                got = [decode.decode_batch_model(data, channels_last=bool(n & 1), **kw),
                       stores[0].render_model(index=index, channels_last=not n & 1, **kw),
                       stores[1].render_model(index=index, channels_last=bool(n & 2), **kw)]
                n += 1
                for j, i in enumerate(index):
                    want = _finish(_ref(i, frames[i][3], mats[j], size, word | (pad == "edge")), MEAN, STD, dtype, flags[j])
                    for g, who in zip(got, ("decode", "store", "compact")):
                        _same(g[j], want, (who, size, dtype, interpolation, clamp, pad, j))


def test_one_matrix_for_all_frames_and_the_plan_calls(frames, stores):
    """One [3, 3] serves every frame; warp_plan reports the window of persp_ref's rule, and a workspace
    of exactly render_model_workspace_bytes() suffices, whatever it held."""
    import torch
    from ccmi import decode
    size = (29, 37)
    m = PR.homography([(0, 0), (37, 0), (37, 29), (0, 29)], [(30, 20), (190, 40), (170, 160), (10, 120)]).astype(np.float32)
    plan = stores[0].warp_plan([0, 1], None, size, perspective=m.reshape(3, 3))
    cplan = stores[0].warp_plan([0, 1], None, size, perspective=m.reshape(3, 3), interpolation="bicubic", pad="edge")
    for j, (_, h, w, _q_) in enumerate(frames):
        assert plan[j]["window"] == PR.window(m, size[0], size[1], h, w, even=j == 0)
        assert cplan[j]["window"] == PR.window(m, size[0], size[1], h, w, even=j == 0, reach=2)
    kw = dict(index=[0, 1], perspective=m.reshape(3, 3), size=size, pad="edge")
    need = stores[0].render_model_workspace_bytes(**kw)
    outs = []
    for byte in (0xA5, 0x5A):
        ws = torch.full((need,), byte, dtype=torch.uint8, device="cuda")
        outs.append(stores[0].render_model(workspace=ws, **kw))
    for j in range(2):
        want = _finish(_ref(j, frames[j][3], m, size, 1))
        _same(outs[0][j], want, ("0xA5", j))
        _same(outs[1][j], want, ("0x5A", j))


# ------------------------------------------------------------------ rows 0 0 1 reproduce affine=
def _affines(frames, index, size):
    places = ((0.31, 0.42, 25, 1.3), (0.0, 0.0, -70, 0.8), (1.0, 1.0, 140, 2.1), (0.5, 0.02, 5, 0.6))
    return np.stack([_mat(_rot(deg, s), (fx * frames[i][2], fy * frames[i][1]), size)
                     for i, (fx, fy, deg, s) in zip(index, places)]).reshape(-1, 2, 3)


@pytest.mark.parametrize("stage", ("plain", "colour", "tone", "blur", "all"))
def test_rows_0_0_1_reproduce_affine(frames, stores, stage):
    """Element for element, in all three dtypes and both interpolations; with a contrast op (the statistics
    pass), tone ops and a blur (the float32 staging) every launch site of the projective kernels is
    crossed.  From the streams and from the store."""
    from ccmi import decode
    index, size = [0, 1, 1, 0], (29, 37)
    aff = _affines(frames, index, size)
    per = np.concatenate([aff, np.broadcast_to(np.array([0, 0, 1], np.float32), (4, 1, 3))], axis=1)
    extra = {"plain": {},
             "colour": dict(colour_ops=[("brightness", 1.2), ("contrast", 1.6), ("saturation", 0.5)]),
             "tone": dict(tone_ops=[("autocontrast", None), ("sharpness", 1.7), ("posterize", 4)]),
             "blur": dict(blur=decode.gaussian_taps(0.9, 5), solarize=0.6),
             "all": dict(colour_ops=[("contrast", 0.7)], tone_ops=[("equalize", None)], blur=decode.gaussian_taps(1.4, 7))}[stage]
    data = [frames[i][0] for i in index]
    for k, dtype in enumerate(_dtypes()):
        for interpolation, clamp in (("bilinear", False), ("bicubic", bool(k & 1))):
            kw = dict(size=size, pad=("fill", "edge")[k & 1], fill=FILL, mean=MEAN, std=STD, dtype=dtype,
                      mirror=[True, False, False, True], channels_last=bool(k == 2), interpolation=interpolation, clamp=clamp,
                      **extra)
            a = decode.decode_batch_model(data, affine=aff, **kw)
            groups = decode.last_tail_groups()
            p = decode.decode_batch_model(data, perspective=per, **kw)
            assert decode.last_tail_groups() == groups
            ra = stores[k & 1].render_model(index=index, affine=aff, **kw)
            rp = stores[k & 1].render_model(index=index, perspective=per, **kw)
            for j in range(4):
                _same(p[j], a[j], ("decode", stage, dtype, interpolation, j))
                _same(rp[j], ra[j], ("store", stage, dtype, interpolation, j))
                _same(rp[j], a[j], ("store against decode", stage, dtype, interpolation, j))
    assert not np.array_equal(_bits(a[0]), _bits(a[3]))


def test_integer_translation_is_the_crop_and_minus_one_the_flip(frames, stores):
    import torch
    from ccmi import decode
    for k, (x, y, w, h) in enumerate(((100, 60, 37, 29), (0, 0, 5, 3), (415, 239, 1, 1))):
        dtype = _dtypes()[k]
        m = np.array([1, 0, x, 0, 1, y, 0, 0, 1], np.float32).reshape(3, 3)
        f = np.array([-1, 0, x + w, 0, 1, y, 0, 0, 1], np.float32).reshape(3, 3)
        for interpolation in ("bilinear", "bicubic"):
            kw = dict(dtype=dtype, output_chroma_format=444, mean=MEAN, std=STD)
            crop = stores[0].render_model(index=[0], roi=(x, y, w, h), **kw)
            flip = stores[0].render_model(index=[0], roi=(x, y, w, h), mirror=True, **kw)
            _same(stores[0].render_model(index=[0], perspective=m, size=(h, w), interpolation=interpolation, **kw)[0], crop[0],
                  ("crop", k, interpolation))
            _same(decode.decode_batch_model([frames[0][0]], perspective=f, size=(h, w), interpolation=interpolation, pad="edge",
                                            **kw)[0], flip[0], ("flip", k, interpolation))


# ------------------------------------------------------------------ placement
def _quad(size, corners):
    """The homography that shows the frame quadrilateral `corners` (tl, tr, br, bl as (x, y)) in the output."""
    oh, ow = size
    return PR.homography([(0, 0), (ow, 0), (ow, oh), (0, oh)], corners).astype(np.float32)


def test_quadrilaterals_that_leave_the_frame_on_each_side_and_outside(frames, stores):
    """On both streams: a trapezoid hanging over each of the four sides, an output wholly outside the frame
    (all fill, or the nearest edge pixel), for both pads and interpolations."""
    from ccmi import decode
    size = (29, 37)
    for i, (data, H, W_, q) in enumerate(frames):
        quads = {"left": [(-60, 20), (90, 50), (80, H - 60), (-40, H - 10)],
                 "right": [(W_ - 90, 30), (W_ + 50, 5), (W_ + 70, H - 20), (W_ - 70, H - 50)],
                 "top": [(40, -50), (W_ - 30, -30), (W_ - 120, 70), (100, 60)],
                 "bottom": [(90, H - 70), (W_ - 100, H - 60), (W_ - 20, H + 40), (10, H + 60)],
                 "outside": [(W_ + 300, -200), (W_ + 420, -190), (W_ + 400, -90), (W_ + 310, -110)]}
        names = list(quads)
        mats = np.stack([_quad(size, quads[k]) for k in names]).reshape(-1, 3, 3)
        for m in mats:
            assert PR.refusal(m, size[0], size[1], H, W_) is None and (m[2, 0] != 0 or m[2, 1] != 0)
        for dtype, (interpolation, clamp, word), pad in zip(_dtypes(), MODES, ("fill", "edge", "fill")):
            kw = dict(perspective=mats, size=size, pad=pad, fill=FILL, mean=MEAN, std=STD, dtype=dtype,
                      interpolation=interpolation, clamp=clamp)
            got = decode.decode_batch_model([data] * len(names), **kw)
            ren = stores[1].render_model(index=[i] * len(names), **kw)
            for j, name in enumerate(names):
                r = _ref(i, q, mats[j], size, word | (pad == "edge"))
                if name == "outside":
                    corner = q[:, 0, W_ - 1]  # the frame's top right pixel is the nearest
                    flat = np.asarray(FILL, np.float32) if pad == "fill" else corner
                    # the blend of equal taps: the weights sum to 1 but for their roundings
                    assert np.abs(r - flat[:, None, None]).max() <= 1e-5
                else:
                    inside = np.abs(r - np.asarray(FILL, np.float32)[:, None, None]).max(axis=0) > 0
                    assert inside.any() and (pad == "edge" or not inside.all())  # part of the output is padding
                want = _finish(r, MEAN, STD, dtype)
                _same(got[j], want, ("decode", i, name, dtype))
                _same(ren[j], want, ("render", i, name, dtype))


def test_a_window_equal_to_the_whole_frame(frames, stores):
    """A quadrilateral around the frame: the plan's window is the frame (the whole-frame tail)."""
    import torch
    from ccmi import decode
    size = (48, 64)
    for i, (data, H, W_, q) in enumerate(frames):
        m = _quad(size, [(-8, -6), (W_ + 5, -12), (W_ + 9, H + 7), (-3, H + 4)])
        assert PR.refusal(m, size[0], size[1], H, W_) is None
        assert stores[0].warp_plan([i], None, size, perspective=m.reshape(3, 3))[0]["window"] == (0, 0, W_, H)
        for dtype, (interpolation, clamp, word) in zip(_dtypes(), MODES):
            kw = dict(perspective=m.reshape(3, 3), size=size, fill=FILL, mean=MEAN, std=STD, dtype=dtype,
                      interpolation=interpolation, clamp=clamp)
            want = _finish(_ref(i, q, m, size, word), MEAN, STD, dtype)
            _same(decode.decode_batch_model([data], **kw)[0], want, ("decode", i, dtype))
            _same(stores[0].render_model(index=[i], **kw)[0], want, ("render", i, dtype))


def test_a_homography_just_inside_the_position_error_bound(frames, stores):
    """The denominator falls to c - 7.5 at the right edge of an 8-wide output; c is the least float32 the
    plan accepts on that frame (E = 7/8 but for one float32 step), and one step below it is refused.  The
    positions run from 0.07 at the left to thousands of pixels at the right edge."""
    from ccmi import decode
    size = (6, 8)
    for i, (data, H, W_, q) in enumerate(frames):
        def make(c):
            return [1, 0, 0, 0, 1, 0, -1, 0, c]
        below, c = _first_with_rank(make, 7.5, 64.0, 3, size[0], size[1], H, W_)
        m = np.asarray(make(c), np.float32)
        assert max(PR.quantities(m, size[0], size[1], H, W_)["E"]) > 0.87
        with pytest.raises(decode.CcmiError, match="too strong"):
            decode.decode_batch_model([data], perspective=np.asarray(make(below), np.float32).reshape(3, 3), size=size)
        for dtype, (interpolation, clamp, word), pad in zip(_dtypes(), MODES, ("edge", "fill", "edge")):
            kw = dict(perspective=m.reshape(3, 3), size=size, pad=pad, fill=FILL, dtype=dtype, interpolation=interpolation,
                      clamp=clamp)
            want = _finish(_ref(i, q, m, size, word | (pad == "edge")), dtype=dtype)
            _same(decode.decode_batch_model([data], **kw)[0], want, ("decode", i, dtype))
            _same(stores[1].render_model(index=[i], **kw)[0], want, ("render", i, dtype))


# ------------------------------------------------------------------ batches
def test_a_frame_is_the_same_alone_and_anywhere_in_a_batch_and_the_groups(frames, stores):
    """Mixed frame sizes and matrices: the same bits alone, in the batch and in the reversed batch; one
    batched tail group per architecture and no per-frame group, as the affine call of the same frames."""
    import torch
    from ccmi import decode
    size = (29, 37)
    index = [0, 1, 1, 0, 0, 1, 0]
    mats = _mats(frames, index, size, 7)
    for dtype, (interpolation, clamp, word) in zip(_dtypes(), MODES):
        kw = dict(size=size, pad="edge", mean=MEAN, std=STD, dtype=dtype, interpolation=interpolation, clamp=clamp)
        whole = stores[0].render_model(index=index, perspective=mats, **kw)
        groups = decode.last_tail_groups()
        stores[0].render_model(index=index, affine=mats[:, :2, :] * 0 + np.array([[1, 0, 3], [0, 1, 2]], np.float32), **kw)
        assert groups == decode.last_tail_groups() and groups[1] == 0 and 1 <= groups[0] <= 2
        back = stores[0].render_model(index=index[::-1], perspective=mats[::-1].copy(), **kw)
        coded = decode.decode_batch_model([frames[i][0] for i in index], perspective=mats, **kw)
        assert decode.last_tail_groups() == groups
        for j, i in enumerate(index):
            alone = stores[0].render_model(index=[i], perspective=mats[j], **kw)
            _same(whole[j], alone[0], ("alone", dtype, j))
            _same(back[len(index) - 1 - j], alone[0], ("reversed", dtype, j))
            _same(coded[j], alone[0], ("coded", dtype, j))
            _same(alone[0], _finish(_ref(i, frames[i][3], mats[j], size, word | 1), MEAN, STD, dtype), ("reference", dtype, j))
    stores[0].render_model(index=[0] * 5, perspective=_mats(frames, [0] * 5, size, 8), size=size, dtype=torch.bfloat16)
    assert decode.last_tail_groups() == (1, 0)


def test_the_per_frame_tail_of_a_stream_without_a_fused_synthesis(gpu, ccmi_lib):
    """The formatted-output tests' generated 21 x 37 stream with a generic synthesis takes the per-frame
    tail (the kernels without _batch): bitwise against the reference, and rows 0 0 1 against affine= with a
    contrast op (the per-frame statistics pass) and a blur (the per-frame staging)."""
    from ccmi import decode
    data = [_generate(21, 37, 11, generic=True)]
    assert not decode.roi_plan(data, (0, 0, 8, 8), output_chroma_format=444)[0]["windowed"]
    planes = _planes(decode.decode_batch(data, output_bitdepth=8, output_chroma_format=444, as_yuv=True)[0], 21, 37, 8, 444)
    q = _q("persp-generic", planes, 8, 444, "rgb")
    size = (13, 11)
    rng = np.random.default_rng(31)
    mats = np.stack(PR.accepted_homographies(rng, 3, 21, 37, size[0], size[1])).reshape(3, 3, 3)
    aff = np.stack([_mat(_rot(33, 1.8), (17, 9), size), _mat(_rot(-20, 0.7), (30, 4), size)]).reshape(2, 2, 3)
    per = np.concatenate([aff, np.broadcast_to(np.array([0, 0, 1], np.float32), (2, 1, 3))], axis=1)
    for dtype, (interpolation, clamp, word), pad in zip(_dtypes(), MODES, ("fill", "edge", "fill")):
        kw = dict(size=size, pad=pad, fill=FILL, mean=MEAN, std=STD, dtype=dtype, output_chroma_format=444,
                  interpolation=interpolation, clamp=clamp)
        got = decode.decode_batch_model(data * 3, perspective=mats, mirror=[False, True, False], **kw)
        assert decode.last_tail_groups() == (0, 3)
        for j in range(3):
            _same(got[j], _finish(_ref("generic", q, mats[j], size, word | (pad == "edge")), MEAN, STD, dtype, j == 1),
                  (dtype, interpolation, j))
        for extra in (dict(colour_ops=[("brightness", 1.2), ("contrast", 1.6)]), dict(blur=decode.gaussian_taps(0.9, 5)),
                      dict(tone_ops=[("autocontrast", None)])):
            a = decode.decode_batch_model(data * 2, affine=aff, **kw, **extra)
            p = decode.decode_batch_model(data * 2, perspective=per, **kw, **extra)
            for j in range(2):
                _same(p[j], a[j], (dtype, interpolation, sorted(extra), j))


# ------------------------------------------------------------------ Python errors
def test_python_errors_and_refusals_leave_the_destination_untouched(frames, stores):
    import torch
    from ccmi import decode
    eye = np.eye(3, dtype=np.float32)
    with pytest.raises(ValueError, match="excludes affine"):
        stores[0].render_model(index=[0], perspective=eye, affine=eye[:2], size=(8, 8))
    with pytest.raises(ValueError, match="needs size"):
        decode.decode_batch_model([frames[0][0]], perspective=eye)
    with pytest.raises(ValueError, match="excludes roi"):
        stores[0].render_model(index=[0], perspective=eye, size=(8, 8), roi=(0, 0, 8, 8))
    out = [torch.full((3, 8, 8), 7.0, device="cuda")]
    for bad, word in (([1, 0, 0, 0, 1, 0, -1, 0, 4], "denominator"), ([1, 0, 0, 0, 1, 0, 0, 0, float("nan")], "finite")):
        with pytest.raises(decode.CcmiError, match=word):
            stores[0].render_model(index=[0], perspective=np.asarray(bad, np.float32).reshape(3, 3), size=(8, 8), out=out)
        assert bool((out[0] == 7.0).all())
