"""tests/tone_ref.py, the numpy restatement of step 3x the GPU tests compare against bit for bit, pinned
against independent torch restatements: equalize's LUT against torchvision's _equalize_single_image written
with bincount / cumsum (integer-equal), autocontrast / posterize / solarize against the same expressions in
torch float32 (bit-equal), sharpness against conv2d within a bound derived here.  torchvision itself is
used where it imports."""
import numpy as np
import pytest
import torch

import tone_ref as T

U = 2.0 ** -24  # the unit roundoff of float32


def _frame(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3, h, w, generator=g, dtype=torch.float32).numpy()


def _tv_lut(q):
    """torchvision's _equalize_single_image on one uint8 channel, as a LUT (None: the image is returned)"""
    hist = torch.bincount(q.reshape(-1), minlength=256)
    nonzero = hist[hist != 0]
    step = torch.div(nonzero[:-1].sum(), 255, rounding_mode="floor")
    if step == 0:
        return None
    lut = torch.div(torch.cumsum(hist, 0) + torch.div(step, 2, rounding_mode="floor"), step, rounding_mode="floor")
    return torch.nn.functional.pad(lut, [1, 0])[:-1].clamp(0, 255)


def _channels():
    g = torch.Generator().manual_seed(5)
    out = {"random": torch.rand(37, 53, generator=g), "constant": torch.full((9, 11), 0.3),
           "constant 0": torch.zeros(4, 4), "constant 1": torch.ones(4, 4),
           "two values": (torch.rand(40, 40, generator=g) < 0.3).float() * 0.6 + 0.2,
           "two values, one pixel": torch.cat([torch.full((300,), 0.25), torch.tensor([0.75])]).view(7, 43),
           "N - H[last] < 255": torch.cat([torch.full((900,), 0.9), torch.rand(200, generator=g) * 0.5]).view(22, 50),
           "N - H[last] = 254": torch.cat([torch.ones(70), torch.rand(254, generator=g) * 0.9]).view(18, 18),
           "N - H[last] = 255": torch.cat([torch.ones(69), torch.rand(255, generator=g) * 0.9]).view(18, 18),
           # k + 0.5 for every k: the quantisation's ties go to even
           "ties": ((torch.arange(255, dtype=torch.float64) + 0.5) / 255.0).float().repeat(3).view(15, 51),
           "narrow": torch.rand(64, 64, generator=g) * 0.1 + 0.45,
           "outside [0, 1]": torch.rand(30, 30, generator=g) * 3.0 - 1.0}
    return out


@pytest.mark.parametrize("name", sorted(_channels()))
def test_equalize_lut_is_torchvisions(name):
    x = _channels()[name].numpy().astype(np.float32)
    q = T.quantise(x)
    assert q.min() >= 0 and q.max() <= 255
    want_q = torch.from_numpy(x).clamp(0, 1).mul(255.0).round().to(torch.int64)  # torch rounds half to even
    assert np.array_equal(q, want_q.numpy())
    hist = np.bincount(q.ravel(), minlength=256)
    lut = T.equalize_lut(hist)
    tv = _tv_lut(want_q)
    if tv is None:
        assert np.array_equal(lut, np.arange(256)), name
        assert q.size - hist[hist.nonzero()[0][-1]] < 255, name
        assert name in ("constant", "constant 0", "constant 1", "N - H[last] < 255", "N - H[last] = 254"), name
    else:
        assert np.array_equal(lut, tv.numpy()), name
    # the op on a frame of this channel: always quantised, also under the identity LUT
    out = T.equalize(np.stack([x, x, x]))
    assert out.dtype == np.float32
    want = (torch.from_numpy(lut)[want_q].to(torch.float32) / 255.0).numpy()
    assert np.array_equal(out[1].view(np.int32), want.view(np.int32)), name


def test_equalize_ties_round_to_even():
    x = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    prod = (x * np.float32(255.0)).astype(np.float64)
    ties = prod == np.arange(255) + 0.5  # the float32 products that land exactly on a tie
    assert ties.sum() > 100
    q = T.quantise(x)
    k = np.arange(255)[ties]
    assert np.array_equal(q[ties], k + (k % 2))


def test_equalize_matches_torchvision_if_it_imports():
    tv = pytest.importorskip("torchvision")
    from torchvision.transforms.v2 import functional as F
    x = torch.from_numpy(_frame(33, 47, 3))
    q = x.mul(255.0).round().to(torch.uint8)
    want = F.equalize(q).float() / 255.0
    got = T.equalize((q.float() / 255.0).numpy())
    assert np.array_equal(got, want.numpy()), tv.__version__


def test_autocontrast_posterize_solarize_are_the_torch_expressions():
    x = torch.from_numpy(_frame(23, 31, 7)) * 1.5 - 0.25  # values outside [0, 1] too
    x[2] = 0.4  # hi == lo: unchanged
    xn = x.numpy()
    # autocontrast
    want = x.clone()
    for c in range(3):
        v = x[c].clamp(0.0, 1.0)
        lo, hi = v.min(), v.max()
        if hi != lo:
            want[c] = ((x[c] - lo) * (torch.tensor(1.0) / (hi - lo))).clamp(0.0, 1.0)
    got = T.autocontrast(xn)
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))
    assert np.array_equal(got[2].view(np.int32), xn[2].view(np.int32))
    # posterize, every bit count
    for b in range(1, 9):
        L = float(2 ** b)
        want = (x.clamp(0.0, 1.0) * L).floor().clamp(0.0, L - 1.0) * torch.tensor(1.0 / L)
        got = T.posterize(xn, b)
        assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32)), b
        assert len(np.unique(got)) <= 2 ** b
    one = T.posterize(np.ones((3, 2, 2), np.float32), 3)
    assert (one == np.float32(7.0 / 8.0)).all()  # 1.0 falls into the top level
    # solarize
    for th in (0.0, 0.5, 1.0, 2.0, float("inf"), -1.0):
        want = torch.where(x >= torch.tensor(th), torch.tensor(1.0) - x, x)
        assert np.array_equal(T.solarize(xn, th).view(np.int32), want.numpy().view(np.int32)), th


def test_clamp_takes_nan_to_zero():
    t = np.array([np.nan, -1.0, 0.25, 2.0, np.inf, -np.inf], dtype=np.float32)
    assert np.array_equal(T.clamp(t), np.array([0, 0, 0.25, 1, 1, 0], dtype=np.float32))


def _conv_f64(x):
    w = torch.full((1, 1, 3, 3), float(T.W_OTHER), dtype=torch.float64)
    w[0, 0, 1, 1] = float(T.W_CENTRE)
    return torch.nn.functional.conv2d(torch.from_numpy(x).double()[:, None], w)[:, 0], float(w.sum())


@pytest.mark.parametrize("size", ((3, 3), (5, 131), (33, 69), (40, 40)))
def test_sharpness_against_conv2d(size):
    """The blurred value b is 9 products and 9 sums from 0.0f of values in [0, 1]: against the exact sum S_b of
    the float32 weights (W = their sum, about 1) each product errs by at most U w x, together U W; the first
    sum, 0 + p, is exact, each of the other 8 by at most U times a partial sum of at most W (1 + 9 U):
    |b - S_b| <= 9 U W (1 + 9 U).  With f = 0 the op returns clamp((0 x) + (1 b)) = clamp(b) exactly.  For a
    factor f, before the clamp: |g| times that, plus U (f + |g| W') for the two products and U (f + |g| W') for
    the sum, W' = W (1 + 9 U)."""
    h, w = size
    x = _frame(h, w, 11)
    exact, W = _conv_f64(x)
    bound_b = 9 * U * W * (1 + 9 * U)
    got = T.sharpness(x, 0.0)
    err = np.abs(got[:, 1:-1, 1:-1].astype(np.float64) - exact.clamp(0, 1).numpy()).max()
    print("sharpness %s: blur error %.3g, bound %.3g" % (size, err, bound_b))
    assert err <= bound_b
    # borders: b = x, so with f = 0 the border is the frame itself, bit for bit
    edge = np.ones((h, w), dtype=bool)
    edge[1:-1, 1:-1] = False
    assert np.array_equal(got[:, edge].view(np.int32), (x + np.float32(0))[:, edge].view(np.int32))
    for f in (0.3, 1.0, 1.9):
        f32 = float(np.float32(f))
        g = float(np.float32(1.0) - np.float32(f))
        Wp = W * (1 + 9 * U)
        bound = abs(g) * bound_b + 2 * U * (f32 + abs(g) * Wp) * (1 + 2 * U)
        want = (f32 * torch.from_numpy(x).double()[:, 1:-1, 1:-1] + g * exact).clamp(0, 1).numpy()
        got = T.sharpness(x, f)
        err = np.abs(got[:, 1:-1, 1:-1].astype(np.float64) - want).max()
        print("sharpness %s f %.1f: error %.3g, bound %.3g" % (size, f, err, bound))
        assert err <= bound
        # the border blends the pixel with itself
        fx = np.float32(f) * x
        gx = (np.float32(1.0) - np.float32(f)) * x
        assert np.array_equal(got[:, edge].view(np.int32), T.clamp(fx + gx)[:, edge].view(np.int32))


@pytest.mark.parametrize("size", ((1, 1), (1, 7), (2, 9), (9, 2), (2, 2)))
def test_sharpness_leaves_frames_of_side_two_or_less(size):
    x = _frame(*size, 13)
    for f in (0.0, 0.5, 1.7):
        assert np.array_equal(T.sharpness(x, f).view(np.int32), x.view(np.int32))


def test_sharpness_matches_torchvision_if_it_imports():
    pytest.importorskip("torchvision")
    from torchvision.transforms.v2 import functional as F
    x = torch.from_numpy(_frame(21, 34, 17))
    for f in (0.0, 0.4, 1.8):
        want = F.adjust_sharpness(x, f).numpy()
        assert np.abs(T.sharpness(x.numpy(), f) - want).max() <= 40 * U


def test_apply_runs_the_ops_in_order_and_matches_colour_ref():
    import colour_ref as R
    x = torch.from_numpy(_frame(17, 29, 19))
    m = np.array([[0.9, 0.2, 0.0, 0.01], [0.1, 0.8, 0.1, 0.0], [0.0, 0.3, 0.7, 0.02]], dtype=np.float32)
    ops = [("brightness", 1.3), ("contrast", 0.6), ("saturation", 1.4), ("matrix", m)]
    assert np.array_equal(T.apply(x, ops).numpy().view(np.int32), R.apply(x, ops).numpy().view(np.int32))
    # two contrasts: each over the frame as it stands (colour_ref takes one per call)
    two = T.apply(x, [("contrast", 1.5), ("brightness", 0.8), ("contrast", 0.5)])
    step = R.apply(R.apply(x, [("contrast", 1.5), ("brightness", 0.8)]), [("contrast", 0.5)])
    assert np.array_equal(two.numpy().view(np.int32), step.numpy().view(np.int32))
    # order matters, and the whole-frame ops see what came before them
    a = T.apply(x, [("equalize", None), ("brightness", 0.5)])
    b = T.apply(x, [("brightness", 0.5), ("equalize", None)])
    assert not np.array_equal(a.numpy(), b.numpy())
    assert np.array_equal(a.numpy(), T.clamp(np.float32(0.5) * T.equalize(x.numpy())))
    assert T.apply(x, []).dtype == torch.float32 and np.array_equal(T.apply(x, []).numpy(), x.numpy())
