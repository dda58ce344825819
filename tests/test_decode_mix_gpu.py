"""The mix stage (ccmi_decode_batch_dev_mix / ccmi_latents_render_mix; decode.decode_batch_model(erase=...,
erase_seed=..., mix=...) and LatentStore.render_model(...)): RandomErasing, MixUp and CutMix in the
decoder's output stage, after the normalisation and before the one rounding to the element type, after the
geometry of all three paths (a region, size=, affine=), the colour ops, the tone ops and the filter.

The reference is never the new code: render_model(float32, mean 0, std 1, the same mirror, the same colour
ops, tone ops, blur and solarize) of the same frames WITHOUT erase / mix, which the earlier stages' tests
pin bit for bit, put through tests/mix_ref.py (steps 4, 4e, 4m restated with torch CPU float32 operations,
pinned by tests/test_decode_mix_ref.py) with the call's scale and bias, then .to(dtype).  Every comparison
is BITWISE, except the drawn values of a noise rectangle, which are held to noise_ref's derived bound.

Streams: those of tests/test_decode_filter_gpu.py -- class D 416 x 240 (420), the generated 21 x 37 streams,
one of them with a generic synthesis (the per-frame tail), and Kodak (RGB).  The mix kernel's tile is 16
rows x 16 groups of 4 pixels (64 columns): the 75 x 141 outputs have a first, interior tiles and a partial
last tile on both axes (rows 16, 16, 16, 16, 11; 36 groups: 16, 16, 4)."""
import numpy as np
import pytest

import mix_ref as M
from test_decode_colour_gpu import FILL, PATHS, ROI, SIZE, _hue, _rot
from test_decode_filter_gpu import _taps, data, store  # noqa: F401  (fixtures)
from test_decode_fmt_gpu import MEAN, STD, _bits, _f32, _same, _sentinel_canvas

pytestmark = pytest.mark.gpu

_BASE, _GROUPS = {}, {}


def _base(store, key, **kw):
    """The float32 render WITHOUT erase / mix (mean 0, std 1) of a call's frames, on the CPU: computed once
    per key, shared and read-only; _GROUPS[key]: the tail groups that call ran."""
    from ccmi import decode
    if key not in _BASE:
        _BASE[key] = store.render_model(**kw).detach().cpu()
        _GROUPS[key] = decode.last_tail_groups()
    return _BASE[key]


def _sb(mean=None, std=None):
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    return [_f32(1.0 / std[c]) for c in range(3)], [_f32(-mean[c] / std[c]) for c in range(3)]


def _check(got, base, what, erase=None, seeds=None, mix=None, mean=None, std=None, dtype=None):
    """every frame of got, bitwise, against mix_ref on base; no noise rectangle in the call"""
    import torch
    scale, bias = _sb(mean, std)
    want, er = M.batch(list(base), scale, bias, erase, seeds, mix)
    for j in range(len(want)):
        assert not er[j].noisy.any()
        _same(got[j], want[j].to(dtype or torch.float32), (what, j))


def _size(path):
    return (ROI[3], ROI[2]) if path == "fmt" else SIZE


def _rect_sets(h, w):
    """1 to 4 rectangles, overlapping (the later one wins), at all four corners, the whole frame, empty, 1 x 1,
    origins 1, 2 and 3 past a multiple of 4 (groups straddle an edge), and an untouched frame"""
    return [[(5, 3, 9, 7, 0.25)],
            [(6, 2, 10, 9, (1.0, -2.0, 3.0)), (10, 6, 9, 8, -0.5)],
            [(0, 0, 3, 2, 0.1), (w - 3, 0, 3, 2, 0.2), (0, h - 2, 3, 2, 0.3), (w - 3, h - 2, 3, 2, 0.4)],
            [(0, 0, w, h, (0.5, 0.6, 0.7))],
            [(7, 5, 0, 4, 9.0), (3, 3, 4, 0, 9.0)],
            [(11, 7, 1, 1, -3.0)],
            [(7, 1, 13, 5, 0.0), (w - 1, h - 1, 1, 1, 2.0), (0, 0, 1, 1, -2.0)],
            None]


@pytest.mark.parametrize("path", sorted(PATHS))
def test_constant_erase(store, path):
    import torch
    from ccmi import decode
    h, w = _size(path)
    erase = _rect_sets(h, w)
    n = len(erase)
    for mirror in ([False] * n, [bool(j % 2 == 0) for j in range(n)]):
        kw = dict(index=[0] * n, mirror=mirror, **PATHS[path])
        base = _base(store, ("erase", path, mirror[0]), **kw)
        assert tuple(base.shape[-2:]) == (h, w)
        got = store.render_model(erase=erase, **kw)
        assert decode.last_tail_groups() == _GROUPS[("erase", path, mirror[0])] == (1, 0)
        _check(got, base, (path, "f32"), erase=erase)
        _same(got[n - 1], base[n - 1], (path, "untouched"))
        for dtype, cl in ((torch.bfloat16, False), (torch.float16, True), (torch.float32, True)):
            got = store.render_model(erase=erase, mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
            _check(got, base, (path, dtype), erase=erase, mean=MEAN, std=STD, dtype=dtype)
            plain = store.render_model(mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
            _same(got[n - 1], plain[n - 1], (path, dtype, "untouched"))  # the call without, bit for bit


@pytest.mark.parametrize("path", sorted(PATHS))
def test_blend_and_box(store, path):
    """Partner before and after the frame, the frame itself, a chain a -> b -> c (b's partner must not enter
    a), lam 0, 1 and 0.3; boxes: interior, the whole frame, 1 x 1, odd origins; a partner-only frame (5) and an
    untouched one (6) in the same call."""
    import torch
    from ccmi import decode
    h, w = _size(path)
    n = 7
    erase = [None, [(2, 1, 6, 5, 4.0)], None, [(9, 3, 5, 4, (0.0, 1.0, -1.0))], None, None, None]
    mixes = ([(1, 0.3), (2, 0.3), (3, 0.0), (3, 0.3), (2, 1.0), None, None],        # 0 -> 1 -> 2 -> 3 -> 3; 4 -> 2
             [(5, (5, 3, 9, 7)), (0, (0, 0, w, h)), (1, (11, 7, 1, 1)), (3, (1, 1, 3, 3)), (5, (w - 5, h - 3, 5, 3)), None, None],
             [(1, 0.75), (0, (3, 5, 7, 9)), None, (5, 0.5), (4, (2, 2, 8, 8)), None, None])
    mirror = [bool(j % 3 == 1) for j in range(n)]
    kw = dict(index=[0] * n, mirror=mirror, **PATHS[path])
    base = _base(store, ("blend", path), **kw)
    for k, mix in enumerate(mixes):
        for dtype, cl in ((torch.float32, False), (torch.bfloat16, True)):
            got = store.render_model(erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
            assert decode.last_tail_groups() == _GROUPS[("blend", path)]
            _check(got, base, (path, k, dtype), erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype)
            plain = store.render_model(mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
            _same(got[6], plain[6], (path, k, dtype, "untouched"))
    got = store.render_model(mix=mixes[0], **kw)  # mean 0, std 1; no erase in the call
    _check(got, base, (path, "unit"), mix=mixes[0])


def test_partners_across_the_batched_and_the_per_frame_tail(store, data):
    """Whole 21 x 37 frames: stream 1 runs the batched tail, stream 2 (generic synthesis) the per-frame tail.
    A per-frame frame is the partner of a batched one and the reverse, blend and box."""
    import torch
    from ccmi import decode
    index = [1, 2, 1, 2, 2]
    erase = [None, [(30, 3, 6, 17, 0.5)], [(0, 0, 3, 21, -1.0)], None, None]
    mix = [(1, 0.3), (0, 0.6), (3, (9, 4, 20, 13)), (2, (1, 1, 35, 19)), None]
    kw = dict(index=index, output_chroma_format=444, mirror=[False, True, False, False, True])
    base = _base(store, "tails", **kw)
    assert tuple(base.shape[-2:]) == (21, 37) and _GROUPS["tails"] == (1, 3)
    for dtype in (torch.float32, torch.float16):
        got = store.render_model(erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype, **kw)
        assert decode.last_tail_groups() == (1, 3)
        _check(got, base, ("tails", dtype), erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype)
    coded = decode.decode_batch_model([data[i] for i in index], erase=erase, mix=mix, mean=MEAN, std=STD, dtype=torch.float16,
                                      **{k: v for k, v in kw.items() if k != "index"})
    assert np.array_equal(_bits(coded), _bits(got))
    # with a blur or a solarize the filter kernel runs in float32 first, per frame (1, 3) and per group (2)
    stages = dict(blur=[None, _taps(3), _taps(2), None, None], solarize=[None, None, 0.5, 0.5, None])
    base = _base(store, "tails filtered", **kw, **stages)
    for dtype in (torch.float32, torch.bfloat16):
        got = store.render_model(erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype, **kw, **stages)
        assert decode.last_tail_groups() == (1, 3)
        _check(got, base, ("tails filtered", dtype), erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_with_colour_ops_tone_ops_blur_and_solarize(store, path):
    """The earlier stages on the taker only (0 <- 1), on the partner only (2 <- 3), on both (4 <- 5), and on a
    frame that erases (6); frame 7 has ops but no part in the mix and keeps the bits of the call without."""
    import torch
    from ccmi import decode
    ops = [("contrast", 1.7), ("matrix", _hue(0.07))]
    tone = [("autocontrast", None), ("sharpness", 1.5), ("posterize", 5)]
    on = [True, False, False, True, True, True, True, True]
    n = len(on)
    cops = [ops if f else [] for f in on]
    tops = [tone if f else [] for f in on]
    blur = [_taps(4) if f else None for f in on]
    sol = [0.5 if f and j != 4 else None for j, f in enumerate(on)]
    erase = [None, [(1, 1, 9, 9, 0.5)], None, None, [(4, 4, 11, 7, -0.5)], None, [(0, 0, 13, 3, (0.1, 0.2, 0.3))], None]
    mix = [(1, 0.3), None, (3, (5, 3, 9, 7)), None, (5, 0.6), None, None, None]
    kw = dict(index=[0] * n, mirror=[bool(j & 1) for j in range(n)], **PATHS[path])
    for name, stages in (("filter", dict(blur=blur, solarize=sol)), ("tone", dict(tone_ops=tops)),
                         ("all", dict(colour_ops=cops, tone_ops=tops, blur=blur, solarize=sol))):
        base = _base(store, ("ops", path, name), **kw, **stages)
        for dtype in (torch.float32, torch.bfloat16):
            got = store.render_model(erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype, **kw, **stages)
            assert decode.last_tail_groups() == _GROUPS[("ops", path, name)] == (1, 0)
            _check(got, base, (path, name, dtype), erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype)
            plain = store.render_model(mean=MEAN, std=STD, dtype=dtype, **kw, **stages)
            _same(got[7], plain[7], (path, name, dtype, "no part in the mix"))


def test_small_outputs(store):
    """1 x 1 and 5 x 7 outputs on all three paths; stream 2 runs the per-frame tail."""
    index = [1, 2, 2, 1]
    for h, w in ((1, 1), (5, 7)):
        erase = [[(0, 0, 1, 1, 0.5)], None, [(w - 1, h - 1, 1, 1, (1.0, 2.0, 3.0))], None]
        mix = [(1, 0.3), (2, (0, 0, w, h)), None, (0, (w // 2, h // 2, 1, 1))]
        geos = {"fmt": dict(roi=(3, 5, w, h)), "size": dict(roi=(3, 5, 17, 11), size=(h, w)),
                "affine": dict(affine=_rot(-30, 1.25, (18.0, 10.0), (h, w)), size=(h, w), fill=FILL)}
        for name, geo in geos.items():
            kw = dict(index=index, output_chroma_format=444, mirror=[False, True, False, True], **geo)
            base = _base(store, ("small", name, h, w), **kw)
            assert tuple(base.shape[-2:]) == (h, w)
            got = store.render_model(erase=erase, mix=mix, mean=MEAN, std=STD, **kw)
            _check(got, base, (name, h, w), erase=erase, mix=mix, mean=MEAN, std=STD)


def test_an_output_of_many_tiles_each_way(store):
    """75 x 141: tiles of 16 rows (16, 16, 16, 16, 11) and of 16 groups (36 groups: 16, 16, 4), from the batched
    tail (a region of the class-D frame) and from the per-frame tail (the generic 21 x 37 stream resampled up);
    bf16 NCHW, fp16 NHWC, and float32 views into a canvas whose rows start 1, 2 and 3 elements off a 16-byte
    boundary (the groups' lead-in), the sentinels around them intact."""
    import torch
    erase = [[(61, 13, 7, 22, 0.5), (63, 31, 66, 18, (1.0, -1.0, 0.0))], None, [(0, 0, 141, 75, 0.25), (127, 63, 14, 12, -2.0)]]
    mix = [(2, 0.3), (0, (62, 15, 67, 50)), None]
    mirror = [False, True, True]
    for name, kw in (("fmt", dict(index=[0] * 3, roi=(100, 60, 141, 75), output_chroma_format=444)),
                     ("size", dict(index=[0, 2, 2], roi=(4, 2, 30, 18), size=(75, 141), output_chroma_format=444))):
        base = _base(store, ("tiles", name), mirror=mirror, **kw)
        assert tuple(base.shape[-2:]) == (75, 141)
        for dtype, cl in ((torch.bfloat16, False), (torch.float16, True)):
            got = store.render_model(erase=erase, mix=mix, mirror=mirror, mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
            _check(got, base, (name, dtype), erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype)
        canvas, pat = _sentinel_canvas((3, 3 * 75 + 9, 141 + 8), torch.float32)
        spots = ((1, 1), (75 + 3, 2), (2 * 75 + 5, 3))
        tiles = [canvas[:, y: y + 75, x: x + 141] for y, x in spots]
        store.render_model(erase=erase, mix=mix, mirror=mirror, mean=MEAN, std=STD, out=tiles, **kw)
        scale, bias = _sb(MEAN, STD)
        want, _ = M.batch(list(base), scale, bias, erase, None, mix)
        mask = np.ones(tuple(canvas.shape), dtype=bool)
        for j, (y, x) in enumerate(spots):
            _same(canvas[:, y: y + 75, x: x + 141], want[j], (name, "tile", j))
            mask[:, y: y + 75, x: x + 141] = False
        assert (_bits(canvas)[mask] == pat).all(), name


@pytest.mark.parametrize("seed", (0, 1, 2 ** 63 + 5))
def test_noise_is_the_contracts_generator_within_the_derived_bound(store, seed):
    """float32; sigma 1 and 0.25 with v non-zero, a constant rectangle over part of the noise.  Every erased
    element within T + 2^-24 (|want| + T) of v_c + noise_ref.gaussian(u1, u2, sigma), none exempt; every other
    element bitwise the reference.  The same frame and seed give the same bits alone, at another position of a
    larger call, mirrored (the index is the stored position) and in NHWC; bf16 is the float32 output rounded."""
    import torch
    rects = [(5, 3, 30, 17, (0.5, -1.5, 2.0), 1.0), (31, 11, 20, 25, (-0.25, 0.75, 1.25), 0.25), (40, 30, 9, 4, 3.0, 0.0)]
    kw = dict(roi=ROI, mean=MEAN, std=STD)
    base = _base(store, "noise", index=[0, 0], mirror=[False, True], roi=ROI)
    scale, bias = _sb(MEAN, STD)
    ref = M.erase(M.normalise(base[0], scale, bias), rects, seed)
    assert int(ref.noisy.sum()) > 3 * 800
    alone = store.render_model(index=[0], erase=[rects], erase_seed=seed, **kw)[0].cpu()
    err = (alone.double() - ref.want).abs()
    assert bool((err[ref.noisy] <= ref.tol[ref.noisy]).all()), float((err - ref.tol)[ref.noisy].max())
    assert np.array_equal(_bits(alone)[~ref.noisy.numpy()], _bits(ref.e)[~ref.noisy.numpy()])
    # batch invariance: position 2 of a call of 4 whose other frames erase with other seeds, mix or do nothing
    erase = [[(0, 0, 64, 48, 0.0, 2.0)], None, rects, [rects[0]]]
    seeds = [seed + 7, 0, seed, seed + 1]
    big = store.render_model(index=[0] * 4, erase=erase, erase_seed=seeds, mix=[None, (0, 0.5), None, None], **kw)
    _same(big[2], alone, "another position")
    nz = ref.noisy.numpy() & np.broadcast_to(M.inside(48, 64, *rects[0][:4]).numpy(), (3, 48, 64))
    assert not np.array_equal(_bits(big[3])[nz], _bits(alone)[nz]), "two seeds give the same draws"
    # mirrored: another frame under the rectangles, the same draws at the same stored positions
    mir = store.render_model(index=[0], erase=[rects], erase_seed=seed, mirror=[True], **kw)[0].cpu()
    ref_m = M.erase(M.normalise(base[1], scale, bias), rects, seed)
    assert np.array_equal(_bits(mir)[ref.noisy.numpy()], _bits(alone)[ref.noisy.numpy()])
    assert np.array_equal(_bits(mir)[~ref.noisy.numpy()], _bits(ref_m.e)[~ref.noisy.numpy()])
    nhwc = store.render_model(index=[0], erase=[rects], erase_seed=seed, channels_last=True, **kw)[0]
    assert tuple(nhwc.stride()) == (1, 64 * 3, 3)
    _same(nhwc, alone, "NHWC")
    bf = store.render_model(index=[0], erase=[rects], erase_seed=seed, dtype=torch.bfloat16, **kw)[0]
    _same(bf, alone.to(torch.bfloat16), "bf16 is the float32 output rounded")
    # one seed for every frame
    both = store.render_model(index=[0, 0], erase=[rects, rects], erase_seed=seed, **kw)
    _same(both[1], alone, "one seed for all")


def test_a_blend_with_a_noise_erased_partner(store):
    """lam a + oml e_p, bitwise, with e_p the device's own float32 output of the unmixed partner; and a box."""
    rects = [(3, 2, 40, 30, (0.5, 0.0, -0.5), 1.0)]
    kw = dict(index=[0, 0, 0], roi=ROI, mirror=[False, True, False])
    base = _base(store, "noisy partner", **kw)
    got = store.render_model(erase=[None, rects, None], erase_seed=[1, 2, 3], mix=[(1, 0.3), None, (1, (1, 1, 50, 40))],
                             mean=MEAN, std=STD, **kw).cpu()
    scale, bias = _sb(MEAN, STD)
    a = [M.normalise(base[j], scale, bias) for j in range(3)]
    _same(got[0], M.blend(a[0], got[1], 0.3), "blend")
    _same(got[2], M.cut(a[2], got[1], (1, 1, 50, 40)), "box")


def test_coded_streams_and_two_chunks(store, data):
    """decode_batch_model equals render_model of a store of the same streams, bitwise; 64 coded streams are the
    smallest call that runs two chunks (partners then cross chunks: the mix launch waits for both)."""
    import torch
    from ccmi import decode
    n = 64
    g = torch.Generator().manual_seed(9)
    erase, seeds = decode.random_erasing(n, (21, 37), p=0.5, value="pixel", generator=g)
    mix, lab = decode.mixup_cutmix(n, (21, 37), pairing="roll", per_frame=True, generator=g)
    assert sum(e is not None for e in erase) > 8 and sum(m is not None for m in mix) > 32
    call = dict(erase=erase, erase_seed=seeds, mix=mix, mean=MEAN, std=STD, dtype=torch.bfloat16, output_chroma_format=444,
                mirror=[bool(j % 5 == 0) for j in range(n)])
    coded = decode.decode_batch_model([data[1]] * n, **call)
    want = store.render_model(index=[1] * n, **call)
    assert np.array_equal(_bits(coded), _bits(want))
    # constant values: the whole call against the reference
    erase = [None if e is None else [r[:4] + (0.5, 0.0) for r in e] for e in erase]
    call.update(erase=erase, erase_seed=None)
    coded = decode.decode_batch_model([data[1]] * n, **call)
    base = _base(store, "chunks", index=[1] * n, output_chroma_format=444, mirror=call["mirror"])
    _check(coded, base, "two chunks", erase=erase, mix=mix, mean=MEAN, std=STD, dtype=torch.bfloat16)
    for path in sorted(PATHS):
        kw = dict(erase=_rect_sets(*_size(path))[:3], mix=[(2, 0.3), (0, (5, 3, 9, 7)), None], mean=MEAN, std=STD,
                  dtype=torch.float16, **PATHS[path])
        assert np.array_equal(_bits(decode.decode_batch_model(data[:1] * 3, **kw)), _bits(store.render_model(index=[0] * 3, **kw)))


def test_no_mix_is_the_call_without_and_the_workspace_follows_the_formula(store):
    import torch
    for path in sorted(PATHS):
        geo = PATHS[path]
        h, w = _size(path)
        kw = dict(index=[0, 0], mean=MEAN, std=STD, dtype=torch.float16, mirror=[False, True], **geo)
        plain = store.render_model(**kw)
        need = store.render_model_workspace_bytes(index=[0, 0], **geo)
        for erase, mix in (([None, None], None), (None, [None, None]), ([[], None], [None, None])):
            got = store.render_model(erase=erase, mix=mix, erase_seed=5, **kw)
            assert np.array_equal(_bits(got), _bits(plain)), (path, erase, mix)
            assert store.render_model_workspace_bytes(index=[0, 0], erase=erase, mix=mix, **geo) == need
        # frame 0 blurred and mixed with frame 1: both staged, one second frame
        frame = -(-12 * h * w // 256) * 256
        grown = store.render_model_workspace_bytes(index=[0, 0], blur=[_taps(3), None], mix=[(1, 0.5), None], **geo)
        staged = store.render_model_workspace_bytes(index=[0, 0], blur=[_taps(3), None], solarize=[None, 1.0], **geo)
        assert grown - staged == 2 * 256 + frame and staged - need == 2 * (frame + 256)
        ws = torch.empty(grown, dtype=torch.uint8, device="cuda")
        a = store.render_model(blur=[_taps(3), None], mix=[(1, 0.5), None], workspace=ws, **kw)
        b = store.render_model(blur=[_taps(3), None], mix=[(1, 0.5), None], **kw)
        assert np.array_equal(_bits(a), _bits(b)), path


def test_zero_strides_and_mix_staged_frames_of_several_sizes(store):
    """ccmi_latents_render_mix itself (the Python calls take one output size): all-zero strides, which resolve
    to EACH frame's own stored size, and mix-staged frames of three sizes in one call, the largest first: two
    pairs and a frame that only erases, one mix launch whose grid covers the largest frame.  Every frame lies
    in a buffer of exactly its own bytes inside a sentinel canvas: its layout is its own and nothing past its
    end, or anywhere else in the canvas, is written."""
    import ctypes as C
    import torch
    from ccmi import check, decode
    L = decode._bind()
    rois = [(100, 60, 64, 48), (36, 20, 64, 48), (8, 4, 20, 24), (200, 100, 20, 24), (4, 4, 12, 10), (40, 40, 30, 18)]
    sizes = [(r[3], r[2]) for r in rois]  # (h, w)
    mirror = [False, True, False, True, False, True]
    erase = [[(5, 3, 9, 7, 0.25)], None, [(1, 1, 6, 5, (1.0, -2.0, 3.0))], None, [(2, 1, 9, 8, -0.5)], None]
    mix = [None, (0, 0.3), (3, (2, 2, 9, 9)), (2, 0.6), None, None]  # frame 5: no part in the mix
    m, idx, rects = store._frames([0] * len(rois), rois)
    fmt, keep = decode._model_fmt(m, "rgb", MEAN, STD, torch.float32, mirror)
    assert (fmt.stride_c, fmt.stride_y, fmt.stride_x) == (0, 0, 0)
    mx, keep_m = decode._mix(erase, None, mix, m)
    head = (store._handle(), idx)
    geom, need = decode._plan_model(store._source(idx), decode._Sink(m, rects, mx=mx, keep=keep_m), fmt, 0, 444)
    assert [(g.height, g.width) for g in geom] == sizes
    slack, offs, pos = 4096, [], 4096
    for h, w in sizes:
        offs.append(pos)
        pos += 3 * h * w + slack
    canvas, pat = _sentinel_canvas((pos,), torch.float32)
    op = (C.c_void_p * m)(*[canvas.data_ptr() + 4 * o for o in offs])
    cap = (C.c_size_t * m)(*[12 * h * w for h, w in sizes])
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    check(L.ccmi_latents_render_mix(*head, m, rects, op, cap, C.byref(fmt), None, None, None, None, None, C.byref(mx), 0, 444,
                                    ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    base = [_base(store, ("sizes", j), index=[0], roi=rois[j], mirror=[mirror[j]], output_chroma_format=444)[0] for j in range(m)]
    scale, bias = _sb(MEAN, STD)
    want, _ = M.batch(base, scale, bias, erase, None, mix)
    mask = np.ones(pos, dtype=bool)
    for j, (h, w) in enumerate(sizes):
        _same(canvas[offs[j]: offs[j] + 3 * h * w].view(3, h, w), want[j], ("sizes", j))
        mask[offs[j]: offs[j] + 3 * h * w] = False
    assert (_bits(canvas)[mask] == pat).all()
