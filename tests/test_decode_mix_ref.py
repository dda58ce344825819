"""tests/mix_ref.py pinned to independent idioms on the CPU -- slice assignment for a constant erase,
roll().mul().add_() for the blend, where() on a box mask for CutMix, the scalar generator for the noise --
and the drawing helpers of ccmi.decode (random_erasing, mixup_cutmix) checked against the ranges their
docstrings state.  No GPU and no library call."""
import math

import numpy as np
import pytest
import torch

import mix_ref
import noise_ref
from ccmi import decode as D

SCALE, BIAS = (1 / 0.229, 1 / 0.224, 1 / 0.225), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225)


def _frames(n, oh, ow, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, oh, ow, generator=g, dtype=torch.float32) for _ in range(n)]


def test_normalise_is_a_rounded_product_then_a_sum():
    y = _frames(1, 5, 7)[0]
    a = mix_ref.normalise(y, SCALE, BIAS)
    for c in range(3):
        s, b = np.float32(SCALE[c]), np.float32(BIAS[c])
        want = (y[c].numpy() * s).astype(np.float32) + b
        assert want.dtype == np.float32 and np.array_equal(a[c].numpy(), want)


def test_constant_erase_is_slice_assignment_and_a_later_rectangle_wins():
    a = _frames(1, 9, 11, 1)[0]
    rects = [(1, 2, 5, 4, 0.25, 0.0), (3, 0, 6, 5, (1.0, -2.0, 3.0), 0.0), (0, 0, 0, 9, 7.0, 0.0), (10, 8, 1, 1, -1.0)]
    got = mix_ref.erase(a, rects)
    want = a.clone()
    want[:, 2:6, 1:6] = 0.25
    want[:, 0:5, 3:9] = torch.tensor([1.0, -2.0, 3.0])[:, None, None]
    want[:, 8:9, 10:11] = -1.0
    assert torch.equal(got.e, want) and not got.noisy.any()
    assert torch.equal(mix_ref.erase(a, None).e, a) and torch.equal(mix_ref.erase(a, []).e, a)
    whole = mix_ref.erase(a, [(0, 0, 11, 9, 0.5)]).e
    assert torch.equal(whole, torch.full_like(a, 0.5))


def test_blend_is_roll_mul_add_and_cut_is_where_on_a_box_mask():
    ys = _frames(4, 6, 10, 2)
    x = torch.stack([mix_ref.normalise(y, SCALE, BIAS) for y in ys])
    for lam in (0.0, 1.0, 0.3, 0.9972972273826599):
        lam32 = float(np.float32(lam))
        rolled = x.roll(1, 0)
        want = rolled.mul(1 - lam32).add_(x.mul(lam32))  # timm / torchvision: x_flipped.mul_(1 - lam); x.mul_(lam).add_(...)
        m, _ = mix_ref.batch(ys, SCALE, BIAS, mixes=[((j - 1) % 4, lam32) for j in range(4)])
        # 1 - lam as a Python float rounds to float32 as 1.0f - lam does: lam is a float32 value
        assert float(np.float32(1 - lam32)) == float(np.float32(1.0) - np.float32(lam32))
        assert torch.equal(torch.stack(m), want)
    box = (3, 1, 4, 2)
    mask = torch.zeros(6, 10, dtype=torch.bool)
    mask[1:3, 3:7] = True
    m, _ = mix_ref.batch(ys, SCALE, BIAS, mixes=[(3 - j, box) for j in range(4)])
    assert torch.equal(torch.stack(m), torch.where(mask, x.flip(0), x))


def test_the_partner_enters_erased_but_unmixed():
    ys = _frames(3, 5, 8, 3)
    erases = [None, [(1, 1, 3, 2, 9.0)], [(0, 0, 8, 5, -4.0)]]
    m, er = mix_ref.batch(ys, SCALE, BIAS, erases=erases, mixes=[(1, 0.25), (2, 0.5), None])  # a chain 0 -> 1 -> 2
    a = [mix_ref.normalise(y, SCALE, BIAS) for y in ys]
    e1 = a[1].clone()
    e1[:, 1:3, 1:4] = 9.0
    assert torch.equal(er[1].e, e1)
    assert torch.equal(m[0], a[0].mul(0.25).add(e1.mul(0.75)))        # frame 1's own partner does not enter
    assert torch.equal(m[1], e1.mul(0.5).add(torch.full_like(e1, -4.0).mul(0.5)))
    assert torch.equal(m[2], torch.full_like(e1, -4.0))
    own, _ = mix_ref.batch(ys[:1], SCALE, BIAS, mixes=[(0, 0.3)])     # a frame may be its own partner
    assert torch.equal(own[0], a[0].mul(float(np.float32(0.3))).add(a[0].mul(float(np.float32(1) - np.float32(0.3)))))


@pytest.mark.parametrize("seed", (0, 1, 2 ** 63 + 5))
def test_noise_follows_the_scalar_generator_at_the_stored_index(seed):
    oh, ow = 5, 7
    a = _frames(1, oh, ow, 4)[0]
    got = mix_ref.erase(a, [(2, 1, 4, 3, (0.5, -0.5, 1.5), 0.25), (0, 0, 3, 2, 1.0, 0.0)], seed)
    v = (0.5, -0.5, 1.5)
    for c in range(3):
        for i in range(oh):
            for k in range(ow):
                const = i < 2 and k < 3
                noise = 1 <= i < 4 and 2 <= k < 6 and not const
                assert bool(got.noisy[c, i, k]) == noise
                if const:
                    assert got.e[c, i, k] == 1.0
                elif noise:
                    u1, u2 = noise_ref.draw_uniforms(seed, 0, 0, (c * oh + i) * ow + k)
                    w = v[c] + float(noise_ref.gaussian(u1, u2, 0.25))
                    assert float(got.want[c, i, k]) == w
                    T = float(noise_ref.gaussian_tol(u1, 0.25))
                    assert float(got.tol[c, i, k]) == T + 2.0 ** -24 * (abs(w) + T)
                else:
                    assert got.e[c, i, k] == a[c, i, k]
    other = mix_ref.erase(a, [(2, 1, 4, 3, (0.5, -0.5, 1.5), 0.25)], seed + 1)
    assert not torch.equal(other.want, got.want)


def test_random_erasing_is_reproducible_and_inside_the_frame():
    H, W = 37, 21
    for value, count in ((0.0, 1), ((0.1, 0.2, 0.3), 3), ("pixel", 2)):
        a = D.random_erasing(200, (H, W), p=0.5, value=value, count=count, generator=torch.Generator().manual_seed(7))
        b = D.random_erasing(200, (H, W), p=0.5, value=value, count=count, generator=torch.Generator().manual_seed(7))
        c = D.random_erasing(200, (H, W), p=0.5, value=value, count=count, generator=torch.Generator().manual_seed(8))
        assert a == b and a[0] != c[0]
        erase, seeds = a
        assert len(erase) == 200 and 60 <= sum(e is not None for e in erase) <= 140   # p = 1/2: 100 +- 5.7 sigma
        for e in erase:
            for x, y, w, h, v, sigma in e or ():
                assert 0 < w < W and 0 < h < H and 0 <= x <= W - w and 0 <= y <= H - h
                assert 0.02 * H * W * 0.5 <= w * h <= 0.33 * H * W * 1.5      # the area, up to the rounding of the sides
                assert (v, sigma) == ((0.0, 1.0) if value == "pixel" else (value, 0.0))
            assert e is None or 1 <= len(e) <= count
        if value == "pixel":
            assert len(seeds) == 200 and all(0 <= s < 2 ** 63 for s in seeds) and len(set(seeds)) == 200
        else:
            assert seeds is None
    assert D.random_erasing(50, (H, W), p=0.0, generator=torch.Generator().manual_seed(1))[0] == [None] * 50
    assert all(e for e in D.random_erasing(50, (H, W), p=1.0, generator=torch.Generator().manual_seed(1))[0])
    # frame j's rectangles do not depend on the frames before it: a fixed number of draws per frame
    long = D.random_erasing(9, (H, W), p=1.0, generator=torch.Generator().manual_seed(3))[0]
    g = torch.Generator().manual_seed(3)
    assert [D.random_erasing(1, (H, W), p=1.0, generator=g)[0][0] for _ in range(9)] == long


def test_mixup_cutmix_is_reproducible_and_label_lam_follows_its_formula():
    H, W, n = 37, 21, 300
    for pairing in ("roll", "flip"):
        a = D.mixup_cutmix(n, (H, W), per_frame=True, pairing=pairing, generator=torch.Generator().manual_seed(5))
        b = D.mixup_cutmix(n, (H, W), per_frame=True, pairing=pairing, generator=torch.Generator().manual_seed(5))
        assert a == b
        mix, lab = a
        cuts = 0
        for j, (e, l) in enumerate(zip(mix, lab)):
            if e is None:
                assert l == 1.0
                continue
            assert e[0] == ((j - 1) % n if pairing == "roll" else n - 1 - j)
            if hasattr(e[1], "__len__"):
                x, y, w, h = e[1]
                assert w > 0 and h > 0 and 0 <= x and x + w <= W and 0 <= y and y + h <= H
                assert l == 1.0 - w * h / float(H * W)
                cuts += 1
            else:
                assert 0.0 <= e[1] <= 1.0 and l == e[1] and float(np.float32(e[1])) == e[1]
        assert 100 <= cuts <= 200  # switch_prob = 1/2: 150 +- 5.8 sigma (less the few empty boxes)
    one = D.mixup_cutmix(8, (H, W), generator=torch.Generator().manual_seed(2))  # one decision for the call
    assert len({None if e is None else e[1] for e in one[0]}) == 1 and len(set(one[1])) == 1
    assert D.mixup_cutmix(8, (H, W), prob=0.0, generator=torch.Generator().manual_seed(2)) == ([None] * 8, [1.0] * 8)
    assert all(not hasattr(e[1], "__len__") for e in D.mixup_cutmix(64, (H, W), cutmix_alpha=0.0, per_frame=True)[0])
    assert all(e is None or hasattr(e[1], "__len__") for e in D.mixup_cutmix(64, (H, W), mixup_alpha=0.0, per_frame=True)[0])


@pytest.mark.parametrize("alpha", (0.8, 1.0, 0.2))
def test_beta_draws_have_the_mean_and_variance_of_beta_a_a(alpha):
    """lam ~ Beta(a, a): mean 1/2, variance 1 / (4 (2a + 1)); N draws at a fixed seed, each moment within 5
    standard errors: of the mean sqrt(var / N), of the variance sqrt((m4 - var^2) / N) with Beta(a, a)'s
    fourth central moment m4 = 3 / (16 (2a + 1) (2a + 3))."""
    N = 20000
    mix, _ = D.mixup_cutmix(N, (8, 8), mixup_alpha=alpha, cutmix_alpha=0.0, per_frame=True,
                            generator=torch.Generator().manual_seed(11))
    lam = np.array([e[1] for e in mix], dtype=np.float64)
    assert lam.size == N and lam.min() >= 0.0 and lam.max() <= 1.0
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    m4 = 3.0 / (16.0 * (2.0 * alpha + 1.0) * (2.0 * alpha + 3.0))
    assert abs(lam.mean() - 0.5) <= 5.0 * math.sqrt(var / N)
    assert abs(lam.var() - var) <= 5.0 * math.sqrt((m4 - var * var) / N)
