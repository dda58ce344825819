"""The blend stage (ccmi_decode_batch_dev_blend / ccmi_latents_render_blend; decode.decode_batch_model(blend=...,
silent=...) and LatentStore.render_model(...)): weighted sums of up to 8 staged frames of a call before the
normalisation and the one rounding (step 3b of ccmi.h), and silent frames that are sources only -- AugMix.

The reference is never the new code: render_model(float32, mean 0, std 1, the same mirror, colour ops, tone
ops, blur and solarize) of the same frames WITHOUT blend, silent, erase and mix, every frame emitting, which
the earlier stages' tests pin bit for bit, put through tests/blend_ref.py (step 3b restated with torch CPU
float32 operations, pinned by tests/test_decode_blend_ref.py, on mix_ref for steps 4 .. 4m) with the call's
scale and bias, then .to(dtype).  Every comparison is BITWISE, no element exempt, except the drawn values of a
noise rectangle (test_noise_rectangles_on_a_blended_frame_and_a_blended_partner), which are held to mix_ref's
derived bound.

Streams: those of tests/test_decode_filter_gpu.py -- class D 416 x 240 (420), the generated 21 x 37 streams,
one of them with a generic synthesis (the per-frame tail), and Kodak (RGB).  The kernel's tile is 16 rows x
16 groups of 4 pixels: the 75 x 141 outputs have a first, interior tiles and a partial last tile both ways."""
import numpy as np
import pytest

import blend_ref as B
from test_decode_colour_gpu import FILL, PATHS, ROI, SIZE, _hue, _rot
from test_decode_filter_gpu import _taps, data, store  # noqa: F401  (fixtures)
from test_decode_fmt_gpu import MEAN, STD, _bits, _f32, _same, _sentinel_canvas

pytestmark = pytest.mark.gpu

_BASE, _GROUPS = {}, {}


def _base(store, key, **kw):
    """The float32 render WITHOUT blend / silent / erase / mix (mean 0, std 1) of a call's frames, all
    emitting, on the CPU: computed once per key, shared and read-only; _GROUPS[key]: its tail groups."""
    from ccmi import decode
    if key not in _BASE:
        _BASE[key] = store.render_model(**kw).detach().cpu()
        _GROUPS[key] = decode.last_tail_groups()
    return _BASE[key]


def _sb(mean=None, std=None):
    mean, std = mean or (0.0,) * 3, std or (1.0,) * 3
    return [_f32(1.0 / std[c]) for c in range(3)], [_f32(-mean[c] / std[c]) for c in range(3)]


def _want(base, blend=None, silent=None, erase=None, mix=None, mean=None, std=None, dtype=None):
    import torch
    scale, bias = _sb(mean, std)
    want, er = B.batch(list(base), scale, bias, blend, silent, erase, None, mix)
    assert not any(e.noisy.any() for e in er)
    return [w.to(dtype or torch.float32) for w in want]


def _check(got, base, what, **kw):
    """every emitted frame of got, bitwise, against blend_ref on base"""
    want = _want(base, **kw)
    assert len(got) == len(want), (what, len(got), len(want))
    for j in range(len(want)):
        _same(got[j], want[j], (what, j))


def _size(path):
    return (ROI[3], ROI[2]) if path == "fmt" else SIZE


def _bright(n):
    """a point tone op per frame, so that the frames of one stream and region differ"""
    return [[("brightness", 0.6 + 0.1 * j)] for j in range(n)]


# 0: the identity; 1: 2 terms; 2: 4 terms, itself among them, one source twice, a negative weight, a sum that is
# not 1; 3: 8 terms with weights 0 and 1 among them; 4: a source that also emits; 5: a silent source; 6: a silent
# frame nobody reads; 7: no part in the blend; 8: one term, a silent frame after it; 9: silent, the last frame
TERMS = [[(0, 1.0)], [(2, 0.5), (3, 0.5)], [(2, 0.25), (4, 0.5), (4, -0.75), (5, 1.5)],
         [(0, 0.0), (1, 1.0), (2, 0.125), (3, -0.3), (4, 0.7), (5, 0.01), (9, 2.0), (3, 0.3)], None, None, None, None,
         [(9, 1.0)], None]
SILENT = [False, False, False, False, False, True, True, False, False, True]


@pytest.mark.parametrize("path", sorted(PATHS))
def test_terms_sources_and_silent_frames(store, path):
    import torch
    from ccmi import decode
    n = len(TERMS)
    kw = dict(index=[0] * n, mirror=[bool(j % 3 == 1) for j in range(n)], tone_ops=_bright(n), **PATHS[path])
    base = _base(store, ("terms", path), **kw)
    assert tuple(base.shape) == (n, 3) + _size(path)
    for dtype, cl in ((torch.float32, False), (torch.bfloat16, False), (torch.float16, True)):
        got = store.render_model(blend=TERMS, silent=SILENT, mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
        assert decode.last_tail_groups() == _GROUPS[("terms", path)] == (1, 0)
        assert tuple(got.shape) == (7, 3) + _size(path)
        _check(got, base, (path, dtype), blend=TERMS, silent=SILENT, mean=MEAN, std=STD, dtype=dtype)
        # K = 1, itself, weight 1: the bits of the frame merely mix-staged (an empty rectangle stages it) ...
        staged = store.render_model(erase=[[(0, 0, 0, 0, 0.0)]] + [None] * (n - 1), mean=MEAN, std=STD, dtype=dtype,
                                    channels_last=cl, **kw)
        _same(got[0], staged[0], (path, dtype, "identity"))
        # ... and a frame with no part in the blend keeps the bits of the call without
        _same(got[5], staged[7], (path, dtype, "no part in the blend"))
    got = store.render_model(blend=TERMS, silent=SILENT, **kw)  # mean 0, std 1
    _check(got, base, (path, "unit"), blend=TERMS, silent=SILENT)


@pytest.mark.parametrize("silent", ([1, 0, 0, 0], [0, 0, 0, 1], [1, 0, 1, 0], [1, 1, 0, 1], [0, 1, 1, 1]))
def test_silent_frames_first_last_interleaved_and_all_but_one(store, silent):
    """Whole 21 x 37 frames of the batched (1) and the per-frame (2) tail; every emitting frame sums all four."""
    import torch
    index = [1, 2, 1, 2]
    silent = [bool(s) for s in silent]
    blend = [None if s else [(k, 0.1 + 0.2 * ((j + k) % 4)) for k in range(4)] for j, s in enumerate(silent)]
    kw = dict(index=index, output_chroma_format=444, mirror=[False, True, True, False], tone_ops=_bright(4))
    base = _base(store, "silent", **kw)
    got = store.render_model(blend=blend, silent=silent, mean=MEAN, std=STD, dtype=torch.bfloat16, **kw)
    assert len(got) == silent.count(False)
    _check(got, base, ("silent", silent), blend=blend, silent=silent, mean=MEAN, std=STD, dtype=torch.bfloat16)
    # out= holds the emitting frames only
    outs = [torch.empty(3, 21, 37, device="cuda") for _ in range(silent.count(False))]
    store.render_model(blend=blend, silent=silent, mean=MEAN, std=STD, out=outs, **kw)
    _check(outs, base, ("silent out=", silent), blend=blend, silent=silent, mean=MEAN, std=STD)


def test_sources_across_chunks_and_across_the_two_tails(store, data):
    """64 coded streams are the smallest call that runs two chunks: equal streams split 32 / 32 in call order,
    and every frame sums frames of the other chunk.  Then, from the store, frames of the batched tail (stream
    1) sum frames of the per-frame tail (stream 2, generic synthesis) and the reverse."""
    import torch
    from ccmi import decode
    n = 64
    blend = [[(j, 0.5), ((j + 32) % n, 0.25), ((j + 37) % n, 0.25)] if j % 4 else None for j in range(n)]
    silent = [j % 4 == 0 and j % 8 != 0 for j in range(n)]
    call = dict(output_chroma_format=444, mirror=[bool(j % 5 == 0) for j in range(n)],
                tone_ops=[[("brightness", 0.5 + j / 64)] for j in range(n)])
    base = _base(store, "chunks", index=[1] * n, **call)
    coded = decode.decode_batch_model([data[1]] * n, blend=blend, silent=silent, mean=MEAN, std=STD, dtype=torch.bfloat16, **call)
    _check(coded, base, "two chunks", blend=blend, silent=silent, mean=MEAN, std=STD, dtype=torch.bfloat16)
    index = [1, 2, 1, 2, 2, 1]
    blend = [[(1, 0.6), (0, 0.4)], [(0, 0.3), (2, 0.3), (4, 0.4)], None, [(5, 1.25), (3, -0.25)], None, None]
    silent = [False, False, True, False, True, True]
    kw = dict(index=index, output_chroma_format=444, mirror=[False, True, False, False, True, True], tone_ops=_bright(6))
    base = _base(store, "tails", **kw)
    assert _GROUPS["tails"] == (1, 3)
    for dtype in (torch.float32, torch.float16):
        got = store.render_model(blend=blend, silent=silent, mean=MEAN, std=STD, dtype=dtype, **kw)
        assert decode.last_tail_groups() == (1, 3)
        _check(got, base, ("tails", dtype), blend=blend, silent=silent, mean=MEAN, std=STD, dtype=dtype)
    coded = decode.decode_batch_model([data[i] for i in index], blend=blend, silent=silent, mean=MEAN, std=STD,
                                      dtype=torch.float16, **{k: v for k, v in kw.items() if k != "index"})
    assert np.array_equal(_bits(coded), _bits(got))


@pytest.mark.parametrize("path", sorted(PATHS))
def test_with_erase_a_blended_partner_and_a_box(store, path):
    """Erase on a blended frame (after the sum and the normalisation); MixUp with a partner that is itself
    blended and erased (it enters with its sum, its rectangles, and not its partner); a CutMix box from a
    blended partner; a silent partner; and tiles away from the box and the rectangles."""
    import torch
    h, w = _size(path)
    n = 7
    blend = [[(0, 0.5), (5, 0.3), (6, 0.2)], [(1, 0.4), (6, 0.6)], None, [(3, 0.7), (5, 0.3)], [(2, 1.0), (4, -0.5)], None, None]
    silent = [False, False, False, False, False, True, True]
    erase = [[(2, 1, 6, 5, 4.0)], [(9, 3, 5, 4, (0.0, 1.0, -1.0)), (0, 0, 3, 3, 0.5)], None, None, [(w - 3, h - 2, 3, 2, -1.0)], None, None]
    mixes = ([(1, 0.3), (0, 0.6), (1, (5, 3, 9, 7)), (5, 0.25), None, None, None],
             [(3, (1, 1, w - 2, h - 2)), (1, 0.5), None, (4, (11, 7, 1, 1)), (6, (0, 0, w, h)), None, None])
    kw = dict(index=[0] * n, mirror=[bool(j % 3 == 1) for j in range(n)], tone_ops=_bright(n), **PATHS[path])
    base = _base(store, ("mix", path), **kw)
    for k, mix in enumerate(mixes):
        for dtype, cl in ((torch.float32, False), (torch.bfloat16, True)):
            got = store.render_model(blend=blend, silent=silent, erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype,
                                     channels_last=cl, **kw)
            _check(got, base, (path, k, dtype), blend=blend, silent=silent, erase=erase, mix=mix, mean=MEAN, std=STD, dtype=dtype)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_colour_ops_tone_ops_and_a_blur_on_individual_sources(store, path):
    """Sources with colour ops, with an equalize and a sharpness chain, with a blur and a solarize (the filter
    kernel then writes the source's second float32 frame), and with none; the clean frame has none."""
    import torch
    from ccmi import decode
    n = 6
    cops = [[], [("contrast", 1.7), ("matrix", _hue(0.07))], [], [], [("brightness", 1.2)], []]
    tops = [[], [], [("equalize", None), ("sharpness", 1.5), ("sharpness", 0.5)], [], [("autocontrast", None), ("posterize", 5)], []]
    blur = [None, None, None, _taps(4), _taps(2), None]
    sol = [None, None, None, 0.5, None, None]
    blend = [[(0, 0.4), (1, 0.15), (2, 0.15), (3, 0.15), (4, 0.15)], None, None, None, None, [(3, 0.5), (4, 0.5)]]
    silent = [False, True, True, True, True, False]
    kw = dict(index=[0] * n, mirror=[True] * 5 + [False], colour_ops=cops, tone_ops=tops, blur=blur, solarize=sol, **PATHS[path])
    base = _base(store, ("stages", path), **kw)
    for dtype in (torch.float32, torch.bfloat16):
        got = store.render_model(blend=blend, silent=silent, mean=MEAN, std=STD, dtype=dtype, **kw)
        assert decode.last_tail_groups() == _GROUPS[("stages", path)] == (1, 0)
        _check(got, base, (path, dtype), blend=blend, silent=silent, mean=MEAN, std=STD, dtype=dtype)


def test_small_outputs_and_an_output_of_many_tiles_each_way(store):
    """1 x 1, 21 x 37 (whole frames) and 75 x 141 outputs (tiles of 16 rows: 16, 16, 16, 16, 11; 36 groups: 16, 16,
    4), from the batched and the per-frame tail; bf16 NCHW, fp16 NHWC, and float32 views into a canvas whose
    rows start 1 and 2 elements off a 16-byte boundary, the sentinels around them intact."""
    import torch
    index = [1, 2, 2, 1, 1]
    blend = [[(0, 0.5), (1, 0.25), (2, 0.25)], None, None, [(4, 0.9), (2, 0.1)], None]
    silent = [False, True, True, False, True]
    mirror = [False, False, True, True, False]
    for h, w, geo in ((1, 1, dict(roi=(3, 5, 17, 11), size=(1, 1))), (21, 37, dict()), (75, 141, dict(roi=(4, 2, 30, 18), size=(75, 141)))):
        kw = dict(index=index, output_chroma_format=444, mirror=mirror, tone_ops=_bright(5), **geo)
        base = _base(store, ("tiles", h, w), **kw)
        assert tuple(base.shape[-2:]) == (h, w)
        erase = [[(w // 2, h // 2, w - w // 2, h - h // 2, 0.5)], None, None, None, None]
        for dtype, cl in ((torch.bfloat16, False), (torch.float16, True)):
            got = store.render_model(blend=blend, silent=silent, erase=erase, mean=MEAN, std=STD, dtype=dtype, channels_last=cl, **kw)
            _check(got, base, (h, w, dtype), blend=blend, silent=silent, erase=erase, mean=MEAN, std=STD, dtype=dtype)
        canvas, pat = _sentinel_canvas((3, 2 * h + 7, w + 8), torch.float32)
        spots = ((1, 1), (h + 3, 2))
        tiles = [canvas[:, y: y + h, x: x + w] for y, x in spots]
        store.render_model(blend=blend, silent=silent, erase=erase, mean=MEAN, std=STD, out=tiles, **kw)
        want = _want(base, blend=blend, silent=silent, erase=erase, mean=MEAN, std=STD)
        mask = np.ones(tuple(canvas.shape), dtype=bool)
        for j, (y, x) in enumerate(spots):
            _same(canvas[:, y: y + h, x: x + w], want[j], (h, w, "tile", j))
            mask[:, y: y + h, x: x + w] = False
        assert (_bits(canvas)[mask] == pat).all(), (h, w)


def test_the_same_bits_alone_elsewhere_in_a_larger_call_and_on_a_second_call(store):
    import torch
    kw = dict(roi=ROI, mean=MEAN, std=STD, dtype=torch.bfloat16)
    tone = _bright(3)
    alone = store.render_model(index=[0] * 3, tone_ops=tone, mirror=[False, True, False], blend=[[(0, 0.5), (1, 0.2), (2, 0.3)], None, None],
                               silent=[False, True, True], **kw)
    assert len(alone) == 1
    # the same three frames at places 4, 2 and 5 of a call of 7 whose other frames blend, mix or do nothing
    tones = [[("brightness", 1.4)], [], tone[1], [("posterize", 3)], tone[0], tone[2], []]
    big = store.render_model(index=[0] * 7, tone_ops=tones, mirror=[True, False, True, False, False, False, True],
                             blend=[[(3, 1.0)], None, None, None, [(4, 0.5), (2, 0.2), (5, 0.3)], None, [(0, 0.5), (6, 0.5)]],
                             silent=[False, False, True, True, False, True, False], mix=[None, (6, 0.5), None, None, None, None, None], **kw)
    assert len(big) == 4
    _same(big[2], alone[0], "another place")
    again = store.render_model(index=[0] * 3, tone_ops=tone, mirror=[False, True, False], blend=[[(0, 0.5), (1, 0.2), (2, 0.3)], None, None],
                               silent=[False, True, True], **kw)
    _same(again[0], alone[0], "a second call")


@pytest.mark.parametrize("seed", (0, 2 ** 63 + 5))
def test_noise_rectangles_on_a_blended_frame_and_a_blended_partner(store, seed):
    """Step 4e's draws in the blend kernel: sigma 1 and 0.25 with v non-zero and a constant rectangle over part of
    the noise, on two frames that are sums (0 and 1; 2 and 3 are silent sources).  Every drawn element within
    mix_ref's bound T + 2^-24 (|want| + T) of v_c + noise_ref.gaussian(u1, u2, sigma), none exempt; every other
    element bitwise.  The same bits at another place of a larger call; MixUp and CutMix with the blended,
    noise-erased partner are bitwise lam a + oml e_p and the box of e_p, e_p the device's own float32 output."""
    import torch
    import mix_ref as M
    rects = [[(5, 3, 30, 17, (0.5, -1.5, 2.0), 1.0), (31, 11, 20, 25, (-0.25, 0.75, 1.25), 0.25), (40, 30, 9, 4, 3.0, 0.0)],
             [(3, 2, 40, 30, (0.5, 0.0, -0.5), 1.0)], None, None]
    seeds = [seed, seed + 1, 0, 0]
    blend = [[(0, 0.5), (2, 0.3), (3, 0.2)], [(1, 0.6), (3, 0.4)], None, None]
    silent = [False, False, True, True]
    tone = _bright(4)
    mirror = [False, True, True, False]
    kw = dict(roi=ROI, mean=MEAN, std=STD)
    base = _base(store, "noise", index=[0] * 4, roi=ROI, tone_ops=tone, mirror=mirror)
    scale, bias = _sb(MEAN, STD)
    want, er = B.batch(list(base), scale, bias, blend, silent, rects, seeds, None)
    got = store.render_model(index=[0] * 4, tone_ops=tone, mirror=mirror, blend=blend, silent=silent, erase=rects,
                             erase_seed=seeds, **kw).cpu()
    assert len(got) == 2
    for j in range(2):
        noisy = er[j].noisy
        assert int(noisy.sum()) > 3 * 500
        err = (got[j].double() - er[j].want).abs()
        assert bool((err[noisy] <= er[j].tol[noisy]).all()), (j, float((err - er[j].tol)[noisy].max()))
        assert np.array_equal(_bits(got[j])[~noisy.numpy()], _bits(want[j])[~noisy.numpy()]), j
    # batch invariance: the same four frames at places 2, 4, 1 and 3 of a call of 6 whose other frames blend or do nothing
    place = [2, 4, 1, 3]
    tones, mirrors, bl, sil, er6, sd6 = [[("brightness", 1.4)]] * 6, [True] * 6, [None] * 6, [False] * 6, [None] * 6, [seed + 9] * 6
    for j, q in enumerate(place):
        tones[q], mirrors[q], sil[q], er6[q], sd6[q] = tone[j], mirror[j], silent[j], rects[j], seeds[j]
        bl[q] = None if blend[j] is None else [(place[s], w) for s, w in blend[j]]
    bl[5], er6[0] = [(0, 0.5), (5, 0.5)], [(0, 0, 64, 48, 0.0, 2.0)]
    big = store.render_model(index=[0] * 6, tone_ops=tones, mirror=mirrors, blend=bl, silent=sil, erase=er6, erase_seed=sd6, **kw)
    assert len(big) == 4
    _same(big[1], got[0], "frame 0 at place 2")
    _same(big[2], got[1], "frame 1 at place 4")
    bf = store.render_model(index=[0] * 4, tone_ops=tone, mirror=mirror, blend=blend, silent=silent, erase=rects, erase_seed=seeds,
                            dtype=torch.bfloat16, channels_last=True, **kw)
    _same(bf[0], got[0].to(bf.dtype), "bf16 NHWC is the float32 output rounded")
    # frame 0 without rectangles mixes with frame 1: the partner enters with its sum and its draws
    exact, _ = B.batch(list(base), scale, bias, blend, silent, None, None, None)
    only1 = [None, rects[1], None, None]
    for what in (0.3, (1, 1, 50, 40)):
        mixed = store.render_model(index=[0] * 4, tone_ops=tone, mirror=mirror, blend=blend, silent=silent, erase=only1,
                                   erase_seed=seeds, mix=[(1, what), None, None, None], **kw).cpu()
        _same(mixed[1], got[1], "the partner itself")
        _same(mixed[0], M.cut(exact[0], mixed[1], what) if hasattr(what, "__len__") else M.blend(exact[0], mixed[1], what), ("mix", what))


def test_no_blend_is_the_mix_call_and_the_workspace_follows_the_formula(store):
    import torch
    for path in sorted(PATHS):
        geo = PATHS[path]
        h, w = _size(path)
        kw = dict(index=[0, 0, 0], mean=MEAN, std=STD, dtype=torch.float16, mirror=[False, True, False], **geo)
        mixed = dict(erase=[[(1, 1, 5, 5, 0.5)], None, None], mix=[None, (0, 0.3), None])
        plain = store.render_model(**kw, **mixed)
        need = store.render_model_workspace_bytes(index=[0, 0, 0], **geo, **mixed)
        for blend, silent in (([None] * 3, None), (None, [False] * 3), ([[], None, []], [False] * 3)):
            got = store.render_model(blend=blend, silent=silent, **kw, **mixed)
            assert np.array_equal(_bits(got), _bits(plain)), (path, blend, silent)
            assert store.render_model_workspace_bytes(index=[0, 0, 0], blend=blend, silent=silent, **geo, **mixed) == need
        # frame 2 joins the two mix-staged frames as a silent source: one more staging frame and mix entry, and the blend table
        frame = -(-12 * h * w // 256) * 256
        grown = store.render_model_workspace_bytes(index=[0, 0, 0], blend=[[(0, 0.5), (2, 0.5)], None, None],
                                                   silent=[False, False, True], **geo, **mixed)
        assert grown - need == frame + 256 + 256 + 256
        ws = torch.empty(grown, dtype=torch.uint8, device="cuda")
        a = store.render_model(blend=[[(0, 0.5), (2, 0.5)], None, None], silent=[False, False, True], workspace=ws, **kw, **mixed)
        b = store.render_model(blend=[[(0, 0.5), (2, 0.5)], None, None], silent=[False, False, True], **kw, **mixed)
        assert np.array_equal(_bits(a), _bits(b)), path


def test_zero_strides_three_sizes_and_null_outputs_of_silent_frames(store):
    """ccmi_latents_render_blend itself (the Python calls take one output size): all-zero strides, which resolve
    to EACH frame's own stored size, blend-staged frames of three sizes in one call, and out_dev[j] = NULL with
    a capacity of 0 for the silent ones.  Every emitting frame lies in a buffer of exactly its own bytes inside
    a sentinel canvas: nothing past its end, or anywhere else in the canvas, is written."""
    import ctypes as C
    import torch
    from ccmi import check, decode
    L = decode._bind()
    rois = [(100, 60, 64, 48), (36, 20, 64, 48), (8, 4, 20, 24), (200, 100, 20, 24), (4, 4, 12, 10), (40, 40, 12, 10), (60, 60, 30, 18)]
    sizes = [(r[3], r[2]) for r in rois]  # (h, w)
    mirror = [False, True, False, True, False, True, False]
    blend = [[(0, 0.5), (1, 0.5)], None, [(3, 1.5), (2, -0.5), (3, 0.25)], None, [(5, 0.3), (5, 0.3), (4, 0.4)], None, None]
    silent = [False, True, False, True, False, True, False]  # frame 6: no part in the blend
    erase = [None, None, [(1, 1, 6, 5, (1.0, -2.0, 3.0))], None, None, None, None]
    m, idx, rects = store._frames([0] * len(rois), rois)
    fmt, keep = decode._model_fmt(m, "rgb", MEAN, STD, torch.float32, mirror)
    assert (fmt.stride_c, fmt.stride_y, fmt.stride_x) == (0, 0, 0)
    mx, keep_m = decode._mix(erase, None, None, m)
    bl, keep_b, quiet = decode._blend(blend, silent, m)
    assert quiet == silent
    geom, need = decode._plan_model(store._source(idx), decode._Sink(m, rects, mx=mx, bl=bl, keep=(keep_m, keep_b)), fmt, 0, 444)
    assert [(g.height, g.width) for g in geom] == sizes  # a silent frame's geometry is filled like any other's
    slack, offs, pos = 4096, [], 4096
    for (h, w), s in zip(sizes, silent):
        offs.append(None if s else pos)
        pos += 0 if s else 3 * h * w + slack
    canvas, pat = _sentinel_canvas((pos,), torch.float32)
    op = (C.c_void_p * m)(*[None if o is None else canvas.data_ptr() + 4 * o for o in offs])
    cap = (C.c_size_t * m)(*[0 if s else 12 * h * w for (h, w), s in zip(sizes, silent)])
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    check(L.ccmi_latents_render_blend(store._handle(), idx, m, rects, op, cap, C.byref(fmt), None, None, None, None, None,
                                      C.byref(bl), C.byref(mx), 0, 444, ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    base = [_base(store, ("sizes", j), index=[0], roi=rois[j], mirror=[mirror[j]], output_chroma_format=444)[0] for j in range(m)]
    scale, bias = _sb(MEAN, STD)
    want, _ = B.batch(base, scale, bias, blend, None, erase, None, None)  # every frame's, the silent ones unused
    mask = np.ones(pos, dtype=bool)
    for j, (h, w) in enumerate(sizes):
        if silent[j]:
            continue
        _same(canvas[offs[j]: offs[j] + 3 * h * w].view(3, h, w), want[j], ("sizes", j))
        mask[offs[j]: offs[j] + 3 * h * w] = False
    assert (_bits(canvas)[mask] == pat).all()


def test_aug_mix_end_to_end(store):
    """aug_mix(width 3) on 8 frames: 32 rendered, 8 returned; crops of the class-D frame as the base matrices,
    a mirror shared by a frame and its chains.  Every frame, clean or chain, is a fused-synthesis frame of one
    geometry: one batched tail group whatever the chains draw."""
    import torch
    from ccmi import decode
    n, size = 8, SIZE
    g = torch.Generator().manual_seed(21)
    crops = np.stack([_rot(0, 0.4 + 0.05 * j, (100.0 + 20 * j, 80.0 + 10 * j), size) for j in range(n)])
    am = decode.aug_mix(n, size, severity=3, mixture_width=3, generator=g, base=crops)
    rep = am["repeat"]
    m = len(rep)
    assert m == 32 and sum(am["silent"]) == 24
    flip = [bool(j % 2) for j in range(n)]
    kw = dict(index=[0] * m, affine=am["matrices"], size=size, fill=FILL, tone_ops=am["tone_ops"], mirror=[flip[r] for r in rep])
    base = _base(store, "augmix", **kw)
    assert _GROUPS["augmix"] == (1, 0)
    for dtype in (torch.float32, torch.bfloat16):
        got = store.render_model(blend=am["blend"], silent=am["silent"], mean=MEAN, std=STD, dtype=dtype, **kw)
        assert decode.last_tail_groups() == (1, 0)
        assert tuple(got.shape) == (n, 3) + size
        _check(got, base, ("augmix", dtype), blend=am["blend"], silent=am["silent"], mean=MEAN, std=STD, dtype=dtype)
    # and MixUp / CutMix of the AugMixed batch: the partner is the blended clean frame of the frame before
    mix = [None] * m
    for j in range(n):
        mix[j * 4] = (((j - 1) % n) * 4, 0.3 if j % 2 else (3, 2, 11, 9))
    got = store.render_model(blend=am["blend"], silent=am["silent"], mix=mix, mean=MEAN, std=STD, dtype=torch.bfloat16, **kw)
    _check(got, base, "augmix mixed", blend=am["blend"], silent=am["silent"], mix=mix, mean=MEAN, std=STD, dtype=torch.bfloat16)
