"""tests/filter_ref.py, the float32 restatement of steps 3y-0 .. 3y-2 of the ccmi_filter contract that the
GPU tests compare the library with bit for bit, pinned here on the CPU: against the same sums in
float64, against F.pad's reflection, against torch.where, and decode.gaussian_taps against torchvision's
formula in float64."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filter_ref

SHAPES = ((1, 1), (2, 3), (5, 7), (21, 37), (33, 65))


def _frame(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3, h, w, generator=g, dtype=torch.float32)


def _taps(r, seed, signed=False):
    g = torch.Generator().manual_seed(100 + seed)
    t = torch.rand(r + 1, generator=g, dtype=torch.float64) + 0.05
    if signed:
        t[1::2] *= -0.5
    full = torch.cat([t[1:].flip(0), t])
    return (t / full.abs().sum() * (1.5 if signed else 1.0)).to(torch.float32).numpy()


@pytest.mark.parametrize("r", (1, 4, 11, 15))
@pytest.mark.parametrize("signed", (False, True))
def test_blur_against_float64(r, signed):
    """Two chained sums of 2r + 1 terms on inputs in [0, 1]: the standard gamma bound of a recursive sum
    of n products is n u per pass relative to sum |w| |x| <= S (u = 2^-24); the second pass works on
    values up to S with weights summing to S again and inherits the first pass's error times S:
    2 (2r + 2) u S^2, taken with the factor 2.1 for the second-order terms.  The clamp is 1-Lipschitz."""
    for k, (h, w) in enumerate(SHAPES):
        x, taps = _frame(h, w, k), _taps(r, k, signed)
        S = float(np.abs(taps[1:].astype(np.float64)).sum() * 2 + abs(float(taps[0])))
        bound = 2.1 * (2 * r + 2) * 2.0 ** -24 * S * S
        got = filter_ref.apply(x, taps)
        err = float((got.double() - filter_ref.blur_f64(x, taps)).abs().max())
        print(f"r {r} {h}x{w} S {S:.3f}: err {err:.3g} bound {bound:.3g}")
        assert got.dtype == torch.float32 and err <= bound
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


def test_refl_is_torch_reflect_padding():
    for n in (2, 3, 5, 7, 37):
        x = torch.arange(n, dtype=torch.float32).view(1, 1, n)
        for r in range(1, min(n - 1, filter_ref.MAX_RADIUS) + 1):  # torch takes a padding below the size
            want = F.pad(x, (r, r), mode="reflect").view(-1).to(torch.int64)
            got = filter_ref.refl(torch.arange(-r, n + r, dtype=torch.int64), n)
            assert torch.equal(got, want), (n, r)
            assert [filter_ref.refl(a, n) for a in range(-r, n + r)] == want.tolist()


def test_refl_folds_where_torch_refuses():
    """period 2 (n - 1), range [0, n), the identity on [0, n), a mirror about 0 and about n - 1"""
    for n in (1, 2, 3, 5, 7):
        a = torch.arange(-3 * filter_ref.MAX_RADIUS, 3 * filter_ref.MAX_RADIUS + n, dtype=torch.int64)
        m = filter_ref.refl(a, n)
        assert int(m.min()) >= 0 and int(m.max()) <= n - 1
        assert torch.equal(filter_ref.refl(torch.arange(n), n), torch.arange(n))
        if n == 1:
            assert int(m.max()) == 0
            continue
        p = 2 * (n - 1)
        assert torch.equal(filter_ref.refl(a + p, n), m) and torch.equal(filter_ref.refl(-a, n), m)
        assert torch.equal(filter_ref.refl(2 * (n - 1) - a, n), m)
    if True:  # torch refuses a padding of the size or more
        with pytest.raises(RuntimeError):
            F.pad(torch.zeros(1, 1, 3), (3, 3), mode="reflect")


@pytest.mark.parametrize("r", (1, 7, 15))
def test_delta_taps_are_the_identity(r):
    taps = np.zeros(r + 1, dtype=np.float32)
    taps[0] = 1.0
    for k, (h, w) in enumerate(SHAPES):
        x = _frame(h, w, 20 + k)
        x[0, 0, 0] = -0.0  # 3y-0: the staged value is + 0.0f
        got = filter_ref.apply(x, taps)
        assert torch.equal(got, x)
        assert not bool(torch.signbit(got).any())
        assert not bool(torch.signbit(filter_ref.apply(x)).any()) and torch.equal(filter_ref.apply(x), x)


def test_solarize_is_torch_where():
    x = _frame(21, 37, 3)
    x[0, 0, :4] = torch.tensor([0.0, 0.5, 1.0, 0.49999997])
    for th in (0.0, 0.5, 1.0, 0.25):
        t32 = torch.tensor(th, dtype=torch.float32)
        want = torch.where(x >= t32, 1.0 - x, x)
        assert torch.equal(filter_ref.apply(x, None, th), want)
    assert torch.equal(filter_ref.apply(x, None, 0.0), 1.0 - x)
    for off in (2.0, 1.0000001, float("inf"), None):  # above 1: off
        assert torch.equal(filter_ref.apply(x, None, off), x)
    # after a blur: on the clamped result
    taps = _taps(4, 0)
    assert torch.equal(filter_ref.apply(x, taps, 0.5), filter_ref.solarize(filter_ref.blur(x, taps), 0.5))
    assert filter_ref.takes_stage(taps, None) and filter_ref.takes_stage(None, 1.0)
    assert not filter_ref.takes_stage(None, 2.0) and not filter_ref.takes_stage(taps[:1], None)


def test_gaussian_taps_against_float64():
    """Every tap within 1e-6 of the float64 formula relative to the kernel (its centre tap, the largest),
    the sum within 1e-6 of 1.  Tap by tap the relative error cannot stay at 1e-6: the exponent
    a = 0.5 (x / sigma)^2 carries the roundings of the division and the square, about 3 u a absolute
    (u = 2^-24), which exp turns into a relative error; with exp's, the sum's and the division's own
    roundings the bound per tap is (3 a + 4) u relative, plus one float32 subnormal step."""
    from ccmi import decode
    u = 2.0 ** -24
    for k in (3, 5, 9, 23, 31):
        for sigma in (0.05, 0.1, 0.37, 1.0, 2.0, 5.0):
            taps = decode.gaussian_taps(sigma, k)
            assert taps.dtype == np.float32 and taps.shape == ((k + 1) // 2,)
            half = (k - 1) * 0.5
            xs = np.linspace(-half, half, k)
            pdf = np.exp(-0.5 * (xs / sigma) ** 2)
            want = (pdf / pdf.sum())[k // 2:]
            err = np.abs(taps.astype(np.float64) - want)
            assert np.all(err <= 1e-6 * want.max()), (k, sigma, err)
            a = 0.5 * (xs[k // 2:] / sigma) ** 2
            assert np.all(err <= (3 * a + 4) * u * want + 2.0 ** -149), (k, sigma, err / np.maximum(want, 1e-300))
            full = float(taps[0]) + 2.0 * float(taps[1:].astype(np.float64).sum())
            assert abs(full - 1.0) <= 1e-6, (k, sigma, full)
    for bad in (0, 4, 33, -3):
        with pytest.raises(ValueError):
            decode.gaussian_taps(1.0, bad)
    with pytest.raises(ValueError):
        decode.gaussian_taps(0.0, 5)


def test_draws_are_seeded():
    from ccmi import decode
    a = decode.gaussian_blur(40, 23, p=0.5, generator=torch.Generator().manual_seed(5))
    b = decode.gaussian_blur(40, 23, p=0.5, generator=torch.Generator().manual_seed(5))
    assert len(a) == 40 and 5 < sum(t is None for t in a) < 35
    assert all((s is None and t is None) or np.array_equal(s, t) for s, t in zip(a, b))
    assert all(t is None or (t.shape == (12,) and t.dtype == np.float32) for t in a)
    s = decode.random_solarize(200, 0.5, 0.2, generator=torch.Generator().manual_seed(6))
    assert s == decode.random_solarize(200, 0.5, 0.2, generator=torch.Generator().manual_seed(6))
    assert 15 < sum(v is not None for v in s) < 70 and all(v in (None, 0.5) for v in s)
    assert all(t is not None for t in decode.gaussian_blur(8, 5, p=1.0, generator=torch.Generator().manual_seed(1)))


def test_filter_argument_shapes():
    from ccmi import decode
    assert decode._filter(None, None, 3) == (None, None)
    t = decode.gaussian_taps(1.0, 5)
    f, (radius, flat, th) = decode._filter(t, None, 3)
    assert radius.tolist() == [2, 2, 2] and flat.size == 10 and th is None and not f.solarize
    f, (radius, flat, th) = decode._filter([None, t, t[:1]], [None, 0.5, 2.0], 3)
    assert radius.tolist() == [0, 2, 0] and np.array_equal(flat[:3], t) and th.tolist() == [2.0, 0.5, 2.0]
    f, (radius, flat, th) = decode._filter(None, 0.25, 2)
    assert radius.tolist() == [0, 0] and th.tolist() == [0.25, 0.25]
    for bad in (([t, t], None), (np.zeros((2, 3), dtype=np.float32), None), (np.zeros(17, dtype=np.float32), None),
                (None, [0.5, 0.5])):
        with pytest.raises(ValueError):
            decode._filter(*bad, 3)
    assert math.isclose(float(t[0] + 2 * t[1:].sum()), 1.0, abs_tol=1e-6)
