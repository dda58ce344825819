"""Pins tests/resample_ref.py, the numpy float32 restatement of the ccmi_resample contract that
tests/test_decode_resample_gpu.py compares the kernels with bit for bit: identity at equal sizes,
and agreement with torch's interpolate(mode="bilinear", antialias=True, align_corners=False)
evaluated in FLOAT64 (torch's own float32 path is up to 1.2e-5 away from its float64 path, so it
is no reference).

The bound: weights w = fl(u / U) carry one rounding each (relative 2^-24, and the exact weights
sum to 1); per pass a value is a sum of T products, each rounded once, accumulated with one
rounding per sum, all values and partial sums in [0, 1].  Weight errors contribute at most
2^-24, the T products together at most 2^-24 (they are bounded by their weights, which sum to
1), the T - 1 roundings of partial sums at most (T - 1) 2^-24: (T + 1) 2^-24 per pass, with a
little slack for the second pass's inputs carrying the first pass's error: (Tx + Ty + 6) 2^-24.
Measured: 1.5e-7 at most."""
import numpy as np
import pytest

import resample_ref as R

SHAPES = ((20, 36, 7, 5), (6, 10, 16, 23), (240, 416, 32, 32), (240, 416, 224, 224), (34, 66, 50, 9),
          (8, 8, 1, 1), (1, 1, 5, 3), (2, 2, 3, 3), (37, 21, 36, 20))  # (h, w, out_h, out_w)


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (3, h, w)).astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("h,w", ((21, 37), (1, 1), (8, 8), (240, 416)))
def test_identity_is_exact(h, w):
    q = _image(h, w, 1)
    assert np.array_equal(R.resample(q, h, w).view(np.int32), q.view(np.int32))
    for i, (j0, ws) in enumerate(R.axis_weights(w, w)):
        assert j0 == i and ws.tolist() == [1.0]


def test_identity_on_one_axis():
    """I == O on one axis only: that pass changes nothing, the other one resamples."""
    q = _image(20, 36, 2)
    a = R.resample(q, 20, 5)
    b = np.stack([R.resample(q[:, y: y + 1, :], 1, 5)[:, 0] for y in range(20)], axis=1)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("h,w,oh,ow", SHAPES)
def test_against_torch_antialiased_bilinear_in_float64(h, w, oh, ow):
    import torch
    q = _image(h, w, 3)
    got = R.resample(q, oh, ow)
    assert got.dtype == np.float32 and got.shape == (3, oh, ow)
    ref = torch.nn.functional.interpolate(torch.from_numpy(q).double()[None], size=(oh, ow), mode="bilinear",
                                          antialias=True, align_corners=False)[0].numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bound = (R.max_taps(w, ow) + R.max_taps(h, oh) + 6) * 2.0 ** -24
    print("%dx%d -> %dx%d: max |diff| %.3g, bound %.3g" % (h, w, oh, ow, err, bound))
    assert err <= bound


def test_tap_counts_of_the_large_downscale():
    """416 x 240 -> 32 x 32 (the GPU test's large case): 25 and 15 taps, counting the
    contract's taps, those with u > 0 (scale 13: the odd 2 j + 1 strictly within 26 of an odd centre)."""
    assert R.max_taps(416, 32) == 25 and R.max_taps(240, 32) == 15


@pytest.mark.parametrize("I,O", ((36, 5), (10, 23), (416, 32), (1, 7), (7, 1), (16384, 1), (1, 16384), (16384, 16383),
                                 (5000, 224), (3, 2), (2, 3)))
def test_tap_run_in_closed_form_and_int32(I, O):
    """The run j0 .. j1 in closed form, as a kernel computes it per thread: with c = (2 i + 1) I
    and D = max(I, O), j0 = floor((c - 2 D - O) / 2 O) + 1 clipped to 0, j1 = floor((c + 2 D - O - 1)
    / 2 O) clipped to I - 1; and every integer involved fits int32 at the contract's 16384."""
    D = max(I, O)
    ws = R.axis_weights(I, O)
    step = max(1, O // 97)
    for i in list(range(0, O, step)) + [O - 1]:
        c = (2 * i + 1) * I
        a, b = c - 2 * D - O, c + 2 * D - O
        j0 = a // (2 * O) + 1 if a >= 0 else 0
        j1 = min((b - 1) // (2 * O), I - 1)
        assert b >= 1 and (j0, j1 - j0 + 1) == (ws[i][0], len(ws[i][1])), (I, O, i)
        big = max(abs(c), abs(a), abs(b), (2 * j1 + 1) * O, 2 * D * (j1 - j0 + 1))
        assert big < 2 ** 31
