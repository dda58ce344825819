"""Pins tests/warp_ref.py, the numpy float32 restatement of the ccmi_warp contract that
tests/test_decode_warp_gpu.py compares the kernels with bit for bit.  400 random rotation / scale /
shear / offset matrices, both pads, on 21 x 37, 34 x 66 and 240 x 416 frames, outputs up to 39 x 39.

Against grid_sample: the float64 evaluation of the definition equals
torch.nn.functional.grid_sample(float64, bilinear, align_corners=False) with the grid in pixels;
CCMI_PAD_FILL is padding_mode="zeros" on q - fill, plus fill, CCMI_PAD_EDGE is "border".  Both
are float64, so they differ by roundings of 1e-16 relative on positions of up to 2^9: 1e-12 holds
(the prototype's largest difference was 4.8e-14).

float32 against float64: at most 4 (3 2^-24 M) + 8 2^-24, M the larger of |m00| out_w +
|m01| out_h + |m02| and the second row's sum, and at least 1.  The float32 position is within
3 2^-24 M of the float64 one per axis (three roundings of values bounded by M); the bilinear
interpolant of values in [0, 1] is continuous with slope at most 1 per axis, across cell borders
and into either padding (fill in [0, 1]); the factor 2 per axis and the 8 roundings of the blend
are slack.  The prototype's worst case was 0.10 of the bound."""
import numpy as np
import pytest

import warp_ref as W

FRAMES = ((21, 37), (34, 66), (240, 416))
FILL = (0.2, 0.5, 0.7)
N_CASES = 400


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (3, h, w)).astype(np.float32) / np.float32(255)


def random_matrix(rng, H, W_, oh, ow):
    """rotation x scale x shear about the output's centre, mapped to a centre in or around the frame"""
    th = rng.uniform(-np.pi, np.pi)
    sx, sy = np.exp(rng.uniform(-1.2, 1.2, 2))
    sh = rng.uniform(-0.5, 0.5)
    A = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[1, sh], [0, 1]]) @ np.diag([sx, sy])
    c = np.array([rng.uniform(-0.3 * W_, 1.3 * W_), rng.uniform(-0.3 * H, 1.3 * H)])
    t = c - A @ np.array([ow / 2, oh / 2])
    return np.concatenate([A[0], t[:1], A[1], t[1:]]).astype(np.float32)


def _cases():
    rng = np.random.default_rng(20240607)
    out = []
    for k in range(N_CASES):
        H, W_ = FRAMES[k % 3]
        oh, ow = (int(v) for v in rng.integers(1, 40, 2))
        out.append((k, H, W_, oh, ow, random_matrix(rng, H, W_, oh, ow)))
    return out


def _grid_sample(q, m, oh, ow, pad):
    import torch
    m = np.asarray(m, np.float32).astype(np.float64)
    H, W_ = q.shape[1:]
    cx, cy = np.arange(ow) + 0.5, np.arange(oh) + 0.5
    xs = m[0] * cx[None, :] + m[1] * cy[:, None] + m[2]
    ys = m[3] * cx[None, :] + m[4] * cy[:, None] + m[5]
    grid = torch.from_numpy(np.stack([2 * xs / W_ - 1, 2 * ys / H - 1], axis=-1))[None]
    x = torch.from_numpy(q.astype(np.float64))[None]
    if pad == W.PAD_EDGE:
        return torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].numpy()
    f = torch.from_numpy(np.asarray(FILL, np.float32).astype(np.float64))[None, :, None, None]  # ccmi_warp::fill is float32
    return (torch.nn.functional.grid_sample(x - f, grid, mode="bilinear", padding_mode="zeros", align_corners=False) + f)[0].numpy()


def test_random_matrices_against_grid_sample_and_float64():
    images = {hw: _image(*hw, seed=5) for hw in FRAMES}
    worst64, worst32, missed = 0.0, 0.0, 0
    for k, H, W_, oh, ow, m in _cases():
        q = images[(H, W_)]
        x, y, w, h = W.window(m, oh, ow, H, W_)
        assert w >= 1 and h >= 1 and 0 <= x and x + w <= W_ and 0 <= y and y + h <= H, (k, (x, y, w, h))
        ty, tx = W.taps_in_frame(m, oh, ow, H, W_)
        missed += int(((tx < x) | (tx >= x + w) | (ty < y) | (ty >= y + h)).sum())
        M = max(W.reach(m, oh, ow), 1.0)
        assert M <= 2.0 ** 22
        bound = 4 * (3 * 2.0 ** -24 * M) + 8 * 2.0 ** -24
        for pad in (W.PAD_FILL, W.PAD_EDGE):
            r64 = W.warp(q, m, oh, ow, pad, FILL, dtype=np.float64)
            ref = _grid_sample(q, m, oh, ow, pad)
            d64 = float(np.abs(r64 - ref).max())
            worst64 = max(worst64, d64)
            assert d64 <= 1e-12, (k, pad, d64)
            r32 = W.warp(q, m, oh, ow, pad, FILL)
            assert r32.dtype == np.float32 and r32.shape == (3, oh, ow)
            d32 = float(np.abs(r32.astype(np.float64) - r64).max())
            worst32 = max(worst32, d32 / bound)
            assert d32 <= bound, (k, pad, d32, bound)
    print("float64 vs grid_sample: %.3g at most; float32 vs float64: %.2f of the bound at most; taps outside their window: %d"
          % (worst64, worst32, missed))
    assert missed == 0


@pytest.mark.parametrize("H,W_", FRAMES)
def test_integer_translation_is_the_crop_and_minus_one_the_flip(H, W_):
    q = _image(H, W_, 9)
    for (x, y, ow, oh) in ((0, 0, W_, H), (3, 5, 8, 8), (W_ - 7, H - 4, 7, 4), (W_ - 1, H - 1, 1, 1)):
        crop = q[:, y: y + oh, x: x + ow]
        for pad in (W.PAD_FILL, W.PAD_EDGE):
            got = W.warp(q, [1, 0, x, 0, 1, y], oh, ow, pad, FILL)
            assert np.array_equal(got.view(np.int32), crop.view(np.int32)), (x, y, ow, oh, pad)
            flip = W.warp(q, [-1, 0, x + ow, 0, 1, y], oh, ow, pad, FILL)
            assert np.array_equal(flip.view(np.int32), crop[:, :, ::-1].view(np.int32)), (x, y, ow, oh, pad)


def test_padding_outside_the_frame():
    """An output wholly outside the frame: all fill, or the nearest corner pixel; the window is
    then one clamped pixel row / column wide and never empty."""
    q = _image(21, 37, 4)
    m = [1, 0, 100, 0, 1, -50]
    f = W.warp(q, m, 4, 6, W.PAD_FILL, FILL)
    assert np.array_equal(f, np.broadcast_to(np.asarray(FILL, np.float32)[:, None, None], (3, 4, 6)))
    e = W.warp(q, m, 4, 6, W.PAD_EDGE)
    assert np.array_equal(e, np.broadcast_to(q[:, 0, 36][:, None, None], (3, 4, 6)))
    assert W.window(m, 4, 6, 21, 37) == (36, 0, 1, 1)
    assert W.window([1, 0, 0, 0, 1, 0], 21, 37, 21, 37) == (0, 0, 37, 21)  # identity at frame size: the frame
    assert W.window([1, 0, 3, 0, 1, 5], 8, 8, 34, 66, even=True) == (2, 4, 12, 12)
