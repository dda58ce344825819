"""Pins tests/cubic_ref.py, the numpy float32 restatement of the bicubic contracts (CCMI_FILTER_CUBIC,
CCMI_WARP_CUBIC) that tests/test_decode_cubic_gpu.py compares the kernels with bit for bit, against
torch evaluated in FLOAT64: interpolate(mode="bicubic", antialias=True, align_corners=False) and
grid_sample(mode="bicubic", align_corners=False, padding_mode zeros / border).

The resize bound is the triangle's (tests/test_decode_resample_ref.py) with the weights' absolute
sums in place of 1.  L = the largest sum_j |w(i, j)| of an axis, T its largest tap count; both are
read off TORCH's float64 weights (the response of interpolate to the unit impulses of one axis),
never off cubic_ref.  The integer weights carry three roundings (two conversions, one division,
relative 3 2^-24 together), a pass's T products one each and its T - 1 partial sums one each, all
bounded by L times the largest input: (T + 3) 2^-24 L per pass on inputs in [0, 1]; the second pass
takes inputs of up to Lx and scales the first pass's error by Ly.  Hence
    (Tx + Ty + 6) Lx Ly 2^-24.
Measured over SHAPES: 0.16 of the bound at most (2.1e-7 absolute at most).

The warp bound, float32 against the same function in float64, M as in tests/test_decode_warp_ref.py:
    26 2^-24 M + 256 2^-24.
Positions: within 3 2^-24 M per axis.  The interpolant is continuous across cells and into either
padding; along an axis its slope is at most max sum_b |k'(t - b)| = 3 (at t = 0, 1; A = -0.75) times
the other axis's sum_a |w_a| <= 1.375 (at t = 0.5) on taps in [0, 1]: 2 axes x 4.125 x 3 2^-24 M < 26
2^-24 M.  Roundings: c_in's five operations leave at most 7 2^-24, c_out's six at most 32 2^-24 (the
error of A s - 5 A is multiplied by s <= 2 twice; the two subtractions of close values are exact),
plus 2 2^-24 from fx + 1 and 1 - fx: 84 2^-24 per tap row on taps in [0, 1], 6 2^-24 more for its
four products and three sums; the second pass scales that by 1.375, adds 84 x 1.375 for its own
coefficients on rows of up to 1.375, and 8 for its products and sums: 124 + 116 + 8 < 256.
Measured over 400 matrices: 0.05 of the bound at most; float64 against grid_sample: 5.2e-14 at most
(1e-11 asserted: float64 roundings of positions of up to 2^9 through a slope of 4.125)."""
import numpy as np
import pytest

import cubic_ref as R
import warp_ref as W
from test_decode_warp_ref import FILL, FRAMES, _cases, _image

SHAPES = ((20, 36, 7, 5), (6, 10, 16, 23), (240, 416, 32, 32), (34, 66, 50, 9), (8, 8, 1, 1), (1, 1, 5, 3),
          (2, 2, 3, 3), (3, 8, 21, 37), (37, 21, 36, 20), (21, 37, 8, 8))  # (h, w, out_h, out_w)
U24 = 2.0 ** -24


def _torch_resize(q, oh, ow):
    import torch
    return torch.nn.functional.interpolate(torch.from_numpy(np.asarray(q, np.float64))[None], size=(oh, ow), mode="bicubic",
                                           antialias=True, align_corners=False)[0].numpy()


_AXIS = {}


def _torch_axis(I, O):
    """(L, T) of an axis from torch's float64 weights: the responses to the I unit impulses."""
    if (I, O) not in _AXIS:
        wts = _torch_resize(np.eye(I)[None], I, O)[0]  # [j, i]: the rows pass is the identity (I == O there)
        _AXIS[(I, O)] = (float(np.abs(wts).sum(axis=0).max()), int((wts != 0).sum(axis=0).max()))
    return _AXIS[(I, O)]


def _resize_bound(h, w, oh, ow):
    (Lx, Tx), (Ly, Ty) = _torch_axis(w, ow), _torch_axis(h, oh)
    assert Lx >= 1 - 1e-12 and Ly >= 1 - 1e-12
    return (Tx + Ty + 6) * Lx * Ly * U24


# ------------------------------------------------------------------ the resize
@pytest.mark.parametrize("h,w,oh,ow", SHAPES)
def test_resize_against_torch_antialiased_bicubic_in_float64(h, w, oh, ow):
    q = _image(h, w, 3)
    got = R.resample(q, oh, ow)
    assert got.dtype == np.float32 and got.shape == (3, oh, ow)
    err = float(np.abs(got.astype(np.float64) - _torch_resize(q, oh, ow)).max())
    bound = _resize_bound(h, w, oh, ow)
    print("%dx%d -> %dx%d: max |diff| %.3g, bound %.3g (%.2f)" % (h, w, oh, ow, err, bound, err / bound))
    assert err <= bound


def test_planted_errors_in_the_resize_break_the_bound():
    """a = -0.75 in place of -0.5, and weights not renormalised where the run is clipped at an edge."""
    for h, w, oh, ow in ((20, 36, 7, 5), (6, 10, 16, 23), (34, 66, 50, 9)):
        q = _image(h, w, 3)
        ref, bound = _torch_resize(q, oh, ow), _resize_bound(h, w, oh, ow)
        assert np.abs(R.resample(q, oh, ow).astype(np.float64) - ref).max() <= bound
        wrong_a = R.resample(q, oh, ow, coef=R.KEYS_075)
        assert np.abs(wrong_a.astype(np.float64) - ref).max() > 100 * bound
        no_renorm = R.resample(q, oh, ow, renorm=False)
        assert np.abs(no_renorm.astype(np.float64) - ref).max() > 100 * bound


def test_weights_for_every_size_pair_up_to_48():
    """U > 0; the taps (n < 2 D2) form one run, the closed form of tap_run; the weights of a run sum
    to 1 within their roundings; the int64 Horner form equals the polynomial in Python ints."""
    for I in range(1, 49):
        for O in range(1, 49):
            D2 = 2 * max(I, O)
            for i in range(O):
                c = (2 * i + 1) * I
                n = [abs((2 * j + 1) * O - c) for j in range(I)]
                taps = [j for j in range(I) if n[j] < 2 * D2]
                j0, j1, lo, hi = R.tap_run(I, O, i)
                assert taps == list(range(j0, j1 + 1)) and taps, (I, O, i)
                assert lo <= j0 and hi >= j1 and (lo == j0 or j0 == 0) and (hi == j1 or j1 == I - 1)
                _, us, U = R.axis_u(I, O, i)
                assert U > 0 and us == [R.u_exact(n[j], D2) for j in taps]
                assert R.u_int64([n[j] for j in taps], D2).tolist() == us
            for j0, ws in R.axis_weights(I, O):
                assert abs(float(ws.astype(np.float64).sum()) - 1.0) <= (len(ws) + 2) * 2 * U24 * float(np.abs(ws).sum())


@pytest.mark.parametrize("I,O", ((16384, 1), (1, 16384), (16384, 16383)))
def test_int64_weights_at_the_extreme_sizes(I, O):
    """The contract's 16384: every int64 value equals Python's unbounded value, every term stays
    below 2^51 and every U below 2^61."""
    D2 = 2 * max(I, O)
    step = max(1, O // 53)
    for i in sorted(set(list(range(0, O, step)) + [O - 1])):
        c = (2 * i + 1) * I
        j0, j1, _, _ = R.tap_run(I, O, i)
        n = [abs((2 * j + 1) * O - c) for j in range(j0, j1 + 1)]
        exact = [R.u_exact(v, D2) for v in n]
        assert R.u_int64(n, D2).tolist() == exact
        assert int(np.asarray(R.u_int64(n, D2)).sum()) == sum(exact) > 0
        assert abs(sum(exact)) < 2 ** 61 and sum(abs(u) for u in exact) < 2 ** 62
        for v in (n[0], n[-1], max(n), min(n)):
            assert max(3 * v ** 3, 5 * v * v * D2, 8 * v * D2 * D2, 4 * D2 ** 3) < 2 ** 51
            assert max(abs((3 * v - 5 * D2) * v * v), abs(((5 * D2 - v) * v - 8 * D2 * D2) * v)) < 2 ** 51


@pytest.mark.parametrize("h,w", ((21, 37), (1, 1), (8, 8), (3, 2)))
def test_resize_identity_is_exact(h, w):
    q = _image(h, w, 1)
    assert np.array_equal(R.resample(q, h, w).view(np.int32), q.view(np.int32))
    for i, (j0, ws) in enumerate(R.axis_weights(w, w)):
        assert ws[i - j0] == 1.0 and float(np.abs(ws).sum()) == 1.0  # the neighbours' u is exactly 0
    a = R.resample(q, h, 5)  # I == O on one axis: that pass changes nothing
    b = np.stack([R.resample(q[:, y: y + 1, :], 1, 5)[:, 0] for y in range(h)], axis=1)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_clamp_moves_only_what_lies_outside():
    q = (_image(8, 8, 5) > 0.5).astype(np.float32)  # black and white: the side lobes overshoot
    r = R.resample(q, 21, 37)
    assert r.min() < 0 and r.max() > 1
    c = R.resample(q, 21, 37, clamp=True)
    inside = (r >= 0) & (r <= 1)
    assert np.array_equal(c[inside].view(np.int32), r[inside].view(np.int32)) and inside.sum() > 0
    assert (c[r < 0] == 0).all() and (c[r > 1] == 1).all() and (~inside).sum() > 0
    m = [0.31, -0.2, 1.7, 0.2, 0.29, 0.4]
    for pad in (R.PAD_FILL, R.PAD_EDGE):
        r = R.warp(q, m, 19, 23, pad, (0.0, 1.0, 0.5))
        assert r.min() < 0 and r.max() > 1
        c = R.warp(q, m, 19, 23, pad, (0.0, 1.0, 0.5), clamp=True)
        inside = (r >= 0) & (r <= 1)
        assert np.array_equal(c[inside].view(np.int32), r[inside].view(np.int32))
        assert (c[r < 0] == 0).all() and (c[r > 1] == 1).all()


# ------------------------------------------------------------------ the warp
def _grid_sample(q, m, oh, ow, pad):
    import torch
    m = np.asarray(m, np.float32).astype(np.float64)
    H, W_ = q.shape[1:]
    cx, cy = np.arange(ow) + 0.5, np.arange(oh) + 0.5
    xs = m[0] * cx[None, :] + m[1] * cy[:, None] + m[2]
    ys = m[3] * cx[None, :] + m[4] * cy[:, None] + m[5]
    grid = torch.from_numpy(np.stack([2 * xs / W_ - 1, 2 * ys / H - 1], axis=-1))[None]
    x = torch.from_numpy(q.astype(np.float64))[None]
    if pad == R.PAD_EDGE:
        return torch.nn.functional.grid_sample(x, grid, mode="bicubic", padding_mode="border", align_corners=False)[0].numpy()
    f = torch.from_numpy(np.asarray(FILL, np.float32).astype(np.float64))[None, :, None, None]
    return (torch.nn.functional.grid_sample(x - f, grid, mode="bicubic", padding_mode="zeros", align_corners=False) + f)[0].numpy()


def _warp_bound(m, oh, ow):
    M = max(W.reach(m, oh, ow), 1.0)
    return 26 * U24 * M + 256 * U24


def test_random_matrices_against_grid_sample_and_float64():
    images = {hw: _image(*hw, seed=5) for hw in FRAMES}
    worst64, worst32, missed = 0.0, 0.0, 0
    for k, H, W_, oh, ow, m in _cases():
        q = images[(H, W_)]
        x, y, w, h = R.window(m, oh, ow, H, W_)
        assert w >= 1 and h >= 1 and 0 <= x and x + w <= W_ and 0 <= y and y + h <= H, (k, (x, y, w, h))
        ty, tx = R.taps_in_frame(m, oh, ow, H, W_)
        missed += int(((tx < x) | (tx >= x + w) | (ty < y) | (ty >= y + h)).sum())
        bound = _warp_bound(m, oh, ow)
        for pad in (R.PAD_FILL, R.PAD_EDGE):
            r64 = R.warp(q, m, oh, ow, pad, FILL, dtype=np.float64)
            d64 = float(np.abs(r64 - _grid_sample(q, m, oh, ow, pad)).max())
            worst64 = max(worst64, d64)
            assert d64 <= 1e-11, (k, pad, d64)
            r32 = R.warp(q, m, oh, ow, pad, FILL)
            assert r32.dtype == np.float32 and r32.shape == (3, oh, ow)
            d32 = float(np.abs(r32.astype(np.float64) - r64).max())
            worst32 = max(worst32, d32 / bound)
            assert d32 <= bound, (k, pad, d32, bound)
    print("float64 vs grid_sample: %.3g at most; float32 vs float64: %.2f of the bound at most; taps outside their window: %d"
          % (worst64, worst32, missed))
    assert missed == 0


def test_planted_error_in_the_warp_breaks_the_bound():
    """A = -0.5 in place of -0.75, on rotations about the frame's centre (every sample off the pixel centres)."""
    q = _image(21, 37, 5)
    for angle, scale in ((0.3, 1.0), (-1.1, 0.6), (2.0, 1.7)):
        c, s = np.cos(angle) / scale, np.sin(angle) / scale
        m = np.array([c, -s, 18.5 - 8 * c + 8 * s, s, c, 10.5 - 8 * s - 8 * c], np.float32)
        for pad in (R.PAD_FILL, R.PAD_EDGE):
            r64 = R.warp(q, m, 16, 16, pad, FILL, dtype=np.float64)
            bound = _warp_bound(m, 16, 16)
            assert np.abs(R.warp(q, m, 16, 16, pad, FILL).astype(np.float64) - r64).max() <= bound
            assert np.abs(R.warp(q, m, 16, 16, pad, FILL, A=-0.5).astype(np.float64) - r64).max() > 100 * bound


@pytest.mark.parametrize("H,W_", FRAMES)
def test_integer_translation_is_the_crop_and_minus_one_the_flip(H, W_):
    q = _image(H, W_, 9)
    for (x, y, ow, oh) in ((0, 0, W_, H), (3, 5, 8, 8), (W_ - 7, H - 4, 7, 4), (W_ - 1, H - 1, 1, 1)):
        crop = q[:, y: y + oh, x: x + ow]
        for pad in (R.PAD_FILL, R.PAD_EDGE):
            got = R.warp(q, [1, 0, x, 0, 1, y], oh, ow, pad, FILL)
            assert np.array_equal(got.view(np.int32), crop.view(np.int32)), (x, y, ow, oh, pad)
            flip = R.warp(q, [-1, 0, x + ow, 0, 1, y], oh, ow, pad, FILL)
            assert np.array_equal(flip.view(np.int32), crop[:, :, ::-1].view(np.int32)), (x, y, ow, oh, pad)
    c = R.coefficients(np.zeros(1, np.float32))
    assert [float(v[0]) for v in c] == [0.0, 1.0, 0.0, 0.0]


def test_padding_outside_the_frame():
    q = _image(21, 37, 4)
    m = [1, 0, 100, 0, 1, -50]
    f = R.warp(q, m, 4, 6, R.PAD_FILL, FILL)
    assert np.array_equal(f, np.broadcast_to(np.asarray(FILL, np.float32)[:, None, None], (3, 4, 6)))
    e = R.warp(q, m, 4, 6, R.PAD_EDGE)
    assert np.array_equal(e, np.broadcast_to(q[:, 0, 36][:, None, None], (3, 4, 6)))
    assert R.window(m, 4, 6, 21, 37) == (36, 0, 1, 1)
    assert R.window([1, 0, 0, 0, 1, 0], 21, 37, 21, 37) == (0, 0, 37, 21)
    assert R.window([1, 0, 3, 0, 1, 5], 8, 8, 34, 66, even=True) == (0, 2, 14, 14)
