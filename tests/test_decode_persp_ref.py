"""Pins tests/persp_ref.py, the numpy float32 restatement of step 3a' of the ccmi_warp contract
(CCMI_WARP_PROJECTIVE) that tests/test_decode_persp_gpu.py compares the kernels with bit for bit.  420
seeded homographies the plan accepts (random quadrilaterals in and around the frame, corners moved by
up to 0.45 of a side, entries scaled by 1, 0.01 or 37) on 21 x 37, 34 x 66 and 240 x 416 frames,
outputs up to 39 x 39, both pads, bilinear and bicubic.

Against grid_sample: the float64 evaluation of the definition equals
torch.nn.functional.grid_sample(float64, align_corners=False) on the projective grid in pixels within
1e-12; CCMI_PAD_FILL is padding_mode="zeros" on q - fill, plus fill, CCMI_PAD_EDGE is "border", as in
tests/test_decode_warp_ref.py.

float32 against float64, bilinear: at most 4 max(E_0, E_1, 3 2^-24) + 8 2^-24.  E_r (ccmi.h) bounds the
float32 position's error on axis r wherever that position lies within two taps of the frame; further
out the interpolant is constant along that axis (fill, or the clamped edge pixel).  The bilinear
interpolant of values in [0, 1] is continuous with slope at most 1 per axis, across cell borders and
into either padding; the factor 2 per axis and the 8 roundings of the blend are slack, as in the affine
file.  Bicubic: at most 9 max(E_0, E_1, 3 2^-24) + 256 2^-24 -- the cubic's slope along an axis is at
most 3 x 1.375 = 4.125 (tests/test_decode_cubic_ref.py), 2 axes x 4.125 = 8.25 < 9, and the 256 2^-24 of
that file's rounding analysis, which does not depend on the positions.
Measured: float64 against grid_sample 2.9e-14 (bilinear) and 3.9e-14 (bicubic) at most; float32 against
float64 0.06 and 0.03 of the bound at most; no tap outside its window."""
import numpy as np
import pytest

import cubic_ref as R
import persp_ref as P
import warp_ref as W
from test_decode_warp_ref import FILL, FRAMES, _cases, _image

N_CASES = 420
U24 = 2.0 ** -24


def _homographies():
    rng = np.random.default_rng(20240911)
    out = []
    for k in range(N_CASES):
        H, W_ = FRAMES[k % 3]
        oh, ow = (int(v) for v in rng.integers(1, 40, 2))
        out.append((k, H, W_, oh, ow, P.accepted_homographies(rng, 1, H, W_, oh, ow)[0]))
    return out


def _grid_sample(q, m, oh, ow, pad, mode):
    import torch
    H, W_ = q.shape[1:]
    xs, ys = P.source(m, oh, ow, np.float64)
    grid = torch.from_numpy(np.stack([2 * xs / W_ - 1, 2 * ys / H - 1], axis=-1))[None]
    x = torch.from_numpy(q.astype(np.float64))[None]
    if pad == P.PAD_EDGE:
        return torch.nn.functional.grid_sample(x, grid, mode=mode, padding_mode="border", align_corners=False)[0].numpy()
    f = torch.from_numpy(np.asarray(FILL, np.float32).astype(np.float64))[None, :, None, None]
    return (torch.nn.functional.grid_sample(x - f, grid, mode=mode, padding_mode="zeros", align_corners=False) + f)[0].numpy()


def test_random_homographies_against_grid_sample_and_float64():
    images = {hw: _image(*hw, seed=5) for hw in FRAMES}
    cases = _homographies()
    assert len(cases) >= 400
    worst64, worst32, missed, projective = [0.0, 0.0], [0.0, 0.0], 0, 0
    for k, H, W_, oh, ow, m in cases:
        q = images[(H, W_)]
        c = P.quantities(m, oh, ow, H, W_)
        assert P.refusal(m, oh, ow, H, W_) is None and c["Dp"] > 0 and max(c["E"]) <= 0.875
        projective += bool(m[6] != 0 or m[7] != 0)
        e = max(c["E"][0], c["E"][1], 3 * U24)
        for ci, (mode, fn, reach, bound) in enumerate((("bilinear", P.warp, 1, 4 * e + 8 * U24),
                                                       ("bicubic", P.cubic, 2, 9 * e + 256 * U24))):
            x, y, w, h = P.window(m, oh, ow, H, W_, reach=reach)
            assert w >= 1 and h >= 1 and 0 <= x and x + w <= W_ and 0 <= y and y + h <= H, (k, (x, y, w, h))
            ty, tx = P.taps_in_frame(m, oh, ow, H, W_, reach)
            missed += int(((tx < x) | (tx >= x + w) | (ty < y) | (ty >= y + h)).sum())
            for pad in (P.PAD_FILL, P.PAD_EDGE):
                r64 = fn(q, m, oh, ow, pad, FILL, dtype=np.float64)
                d64 = float(np.abs(r64 - _grid_sample(q, m, oh, ow, pad, mode)).max())
                worst64[ci] = max(worst64[ci], d64)
                assert d64 <= 1e-12, (k, mode, pad, d64)
                r32 = fn(q, m, oh, ow, pad, FILL)
                assert r32.dtype == np.float32 and r32.shape == (3, oh, ow)
                d32 = float(np.abs(r32.astype(np.float64) - r64).max())
                worst32[ci] = max(worst32[ci], d32 / bound)
                assert d32 <= bound, (k, mode, pad, d32, bound)
    print("float64 vs grid_sample: %.3g (bilinear) %.3g (bicubic) at most; float32 vs float64: %.2f and %.2f of the "
          "bound at most; taps outside their window: %d; matrices with a projective row: %d"
          % (worst64[0], worst64[1], worst32[0], worst32[1], missed, projective))
    assert missed == 0
    assert projective >= 300  # strength 0 of the generator is an affine quadrilateral


def test_the_patched_positions_are_restored():
    q = _image(21, 37, 3)
    P.warp(q, P.as9([1, 0, 2, 0, 1, 3]), 4, 4)
    assert W.positions.__module__ == "warp_ref" and W.positions.__name__ == "positions"


def test_last_row_0_0_1_is_the_affine_reference_bit_for_bit():
    """wn is exactly 1 and the quotient exact: warp_ref / cubic_ref, and their windows."""
    images = {hw: _image(*hw, seed=6) for hw in FRAMES}
    for k, H, W_, oh, ow, m6 in _cases()[:120]:
        q, m9 = images[(H, W_)], P.as9(m6)
        for pad in (P.PAD_FILL, P.PAD_EDGE):
            a, b = P.warp(q, m9, oh, ow, pad, FILL), W.warp(q, m6, oh, ow, pad, FILL)
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (k, pad)
            for clamp in (False, True):
                a, b = P.cubic(q, m9, oh, ow, pad, FILL, clamp), R.warp(q, m6, oh, ow, pad, FILL, clamp)
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (k, pad, clamp)
        for even in (False, True):
            assert P.window(m9, oh, ow, H, W_, even) == W.window(m6, oh, ow, H, W_, even)
            assert P.window(m9, oh, ow, H, W_, even, reach=2) == R.window(m6, oh, ow, H, W_, even)
        # every affine call accepted today stays acceptable: E <= 0.77 at the reach limit
        assert P.refusal(m9, oh, ow, H, W_) is None
    # ... but for the last 3 2^-24 of the reach: D' = 1 - 3 2^-24 there, and S / D' <= 2^22 is the check
    assert P.refusal(P.as9([0, 0, 2.0 ** 22, 0, 0, 1]), 39, 39, 240, 416) == "2^22"
    top = P.as9([0, 0, 2.0 ** 22 - 1, 0, 0, -(2.0 ** 22 - 1)])
    assert P.refusal(top, 39, 39, 240, 416) is None and max(P.quantities(top, 39, 39, 240, 416)["E"]) <= 0.77
    # the largest frame a header can state
    assert max(P.quantities(top, 16384, 16384, 65535, 65535)["E"]) <= 0.77


@pytest.mark.parametrize("H,W_", FRAMES)
def test_integer_translation_is_the_crop_and_minus_one_the_flip(H, W_):
    q = _image(H, W_, 9)
    for (x, y, ow, oh) in ((0, 0, W_, H), (3, 5, 8, 8), (W_ - 1, H - 1, 1, 1)):
        crop = q[:, y: y + oh, x: x + ow]
        for fn in (P.warp, P.cubic):
            got = fn(q, [1, 0, x, 0, 1, y, 0, 0, 1], oh, ow, P.PAD_EDGE)
            assert np.array_equal(got.view(np.int32), crop.view(np.int32))
            flip = fn(q, [-1, 0, x + ow, 0, 1, y, 0, 0, 1], oh, ow, P.PAD_FILL, FILL)
            assert np.array_equal(flip.view(np.int32), crop[:, :, ::-1].view(np.int32))


def test_perspective_matrix_sends_the_endpoints_to_the_startpoints():
    from ccmi import decode
    rng = np.random.default_rng(3)
    for H, W_ in FRAMES + ((720, 1280),):
        for _ in range(50):
            oh, ow = (int(v) for v in rng.integers(8, 300, 2))
            ends = np.array([[0, 0], [ow, 0], [ow, oh], [0, oh]], float) + rng.uniform(-0.2, 0.2, (4, 2)) * [ow, oh]
            starts = np.array([[0, 0], [W_, 0], [W_, H], [0, H]], float) + rng.uniform(-0.3, 0.3, (4, 2)) * [W_, H]
            m32 = decode.perspective_matrix(starts, ends)
            assert m32.dtype == np.float32 and m32.shape == (3, 3) and m32[2, 2] == 1
            m = decode._perspective_f64(starts, ends)
            assert np.array_equal(m.astype(np.float32), m32)
            for e, s in zip(ends, starts):
                v = m @ [e[0], e[1], 1.0]
                assert np.abs(v[:2] / v[2] - s).max() <= 1e-9 * max(H, W_), (H, W_, e, s)
    # the identity, and persp_ref's own solver
    sq = [(0, 0), (7, 0), (7, 5), (0, 5)]
    assert np.array_equal(decode.perspective_matrix(sq, sq), np.eye(3, dtype=np.float32))
    assert np.allclose(P.homography(ends, starts).reshape(3, 3), m, rtol=0, atol=1e-9 * np.abs(m).max())
    with pytest.raises(ValueError):
        decode.perspective_matrix([(0, 0), (1, 1), (2, 2), (3, 3)], sq)
    with pytest.raises(ValueError):
        decode.perspective_matrix(sq[:3], sq[:3])


def test_random_perspective_draws_lie_in_the_stated_ranges():
    """The matrix sends each drawn endpoint to an image corner, so the inverse map of the corners gives the
    draws back: integers in the docstring's ranges."""
    from ccmi import decode
    for (h, w), d in (((224, 224), 0.5), ((37, 21), 0.6), ((64, 48), 0.0)):
        mats = decode.random_perspective(300, (h, w), distortion_scale=d, p=1.0, generator=11)
        assert mats.dtype == np.float32 and mats.shape == (300, 3, 3)
        hh, hw = int(d * h / 2), int(d * w / 2)
        lo = np.array([[0, 0], [w - hw - 1, 0], [w - hw - 1, h - hh - 1], [0, h - hh - 1]])
        hi = np.array([[hw, hh], [w - 1, hh], [w - 1, h - 1], [hw, h - 1]])
        seen = np.zeros((4, 2, 2), bool)
        for m in mats:
            inv = np.linalg.inv(m.astype(np.float64))
            for c, corner in enumerate(((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1))):
                v = inv @ [corner[0], corner[1], 1.0]
                e = v[:2] / v[2]
                assert np.abs(e - np.rint(e)).max() <= 1e-3, (m, e)
                e = np.rint(e)
                assert (e >= lo[c]).all() and (e <= hi[c]).all(), (c, e, lo[c], hi[c])
                seen[c, :, 0] |= e == lo[c]
                seen[c, :, 1] |= e == hi[c]
        assert seen.all()  # both ends of every range are drawn
    assert np.array_equal(decode.random_perspective(5, (8, 8), p=0.0, generator=1), np.broadcast_to(np.eye(3, dtype=np.float32), (5, 3, 3)))


def test_random_perspective_probability_base_and_seed():
    from ccmi import decode
    n, ident = 4000, np.eye(3, dtype=np.float32)
    for p in (0.5, 0.2):
        mats = decode.random_perspective(n, (224, 224), p=p, generator=5)
        share = sum(not np.array_equal(m, ident) for m in mats) / n
        # a drawn frame is the identity only if all four corners fall on the image's: 113^-8
        assert abs(share - p) <= 4 * np.sqrt(p * (1 - p) / n), (p, share)
    a = decode.random_perspective(16, (32, 48), generator=9)
    assert np.array_equal(a, decode.random_perspective(16, (32, 48), generator=np.random.default_rng(9)))
    base = np.stack([decode.affine_matrix((32, 48), (100.0 + j, 60.0), angle=0.1 * j, scale=0.5) for j in range(16)])
    b = decode.random_perspective(16, (32, 48), base=base, generator=9)
    for j in range(16):
        want = np.vstack([base[j].astype(np.float64), [0, 0, 1]]) @ a[j].astype(np.float64)
        assert np.allclose(b[j], want, rtol=1e-5, atol=1e-5) and b[j][2, 2] == 1
    one = decode.random_perspective(16, (32, 48), base=base[3], generator=9)
    assert np.array_equal(one[3], b[3])
    with pytest.raises(ValueError):
        decode.random_perspective(4, (8, 8), base=np.zeros((3, 2, 3)))
    with pytest.raises(ValueError):
        decode.random_perspective(4, (8, 8), distortion_scale=1.5)
