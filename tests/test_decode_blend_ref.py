"""tests/blend_ref.py pinned to an independent idiom (an explicit per-element numpy float32 loop), and the
draws of decode.aug_mix() / decode.auto_augment() held to the ranges their docstrings state.  CPU only."""
import numpy as np
import torch

import blend_ref as B

F = np.float32


def _frames(n, h=5, w=7, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, h, w, generator=g, dtype=torch.float32) * 1.5 - 0.25 for _ in range(n)]


def test_weighted_sum_is_the_per_element_float32_loop():
    ys = _frames(4)
    lists = ([(0, 1.0)], [(1, 0.5), (2, 0.5)], [(3, 0.3), (3, 0.3), (0, -1.7), (1, 0.0)],
             [(j % 4, 0.1 * (j + 1)) for j in range(8)], [(2, 1e-3), (1, 3.0), (2, 1.0 / 3.0)])
    for terms in lists:
        got = B.weighted_sum(ys, terms).numpy()
        for c in range(3):
            for i in range(5):
                for k in range(7):
                    z = None
                    for s, w in terms:
                        p = F(F(w) * F(ys[s][c, i, k].item()))  # the product rounded ...
                        z = p if z is None else F(z + p)          # ... before the sum
                    assert got[c, i, k].view(np.int32) == z.view(np.int32), (terms, c, i, k)
    one = B.weighted_sum(ys, [(2, 1.0)])
    assert np.array_equal(one.numpy().view(np.int32), ys[2].numpy().view(np.int32))  # the identity


def test_batch_blends_before_the_normalisation_and_a_partner_enters_blended():
    ys = _frames(4)
    scale, bias = [F(1 / 0.229).item(), F(1 / 0.224).item(), F(1 / 0.225).item()], [F(-2.1).item(), F(-2.0).item(), F(-1.8).item()]
    blend = [[(0, 0.5), (1, 0.25), (2, 0.25)], None, None, [(3, 0.6), (1, 0.4)]]
    silent = [False, True, False, False]
    erase = [None, None, None, [(1, 1, 3, 2, 0.5)]]
    mix = [(3, 0.3), None, None, None]
    out, _ = B.batch(ys, scale, bias, blend, silent, erase, None, mix)
    assert len(out) == 3
    lam, oml = F(0.3), F(1.0) - F(0.3)
    for c in range(3):
        for i in range(5):
            for k in range(7):
                v = lambda j: F(ys[j][c, i, k].item())  # noqa: E731
                z0 = F(F(F(F(0.5) * v(0)) + F(F(0.25) * v(1))) + F(F(0.25) * v(2)))
                z3 = F(F(F(0.6) * v(3)) + F(F(0.4) * v(1)))
                a0 = F(F(z0 * F(scale[c])) + F(bias[c]))
                a3 = F(F(z3 * F(scale[c])) + F(bias[c]))
                if 1 <= k < 4 and 1 <= i < 3:
                    a3 = F(0.5)
                m0 = F(F(lam * a0) + F(oml * a3))
                a2 = F(F(v(2) * F(scale[c])) + F(bias[c]))
                assert out[0][c, i, k].numpy().view(np.int32) == m0.view(np.int32)
                assert out[1][c, i, k].numpy().view(np.int32) == a2.view(np.int32)
                assert out[2][c, i, k].numpy().view(np.int32) == a3.view(np.int32)


def test_aug_mix_draws_stay_inside_the_documented_ranges():
    from ccmi import decode
    size = (48, 64)
    names = {"brightness", "saturation", "contrast", "sharpness", "posterize", "solarize", "autocontrast", "equalize"}
    for severity, width, depth, all_ops in ((3, 3, -1, True), (10, 7, 3, True), (1, 1, 1, False), (5, 2, -1, False)):
        n = 40
        r = decode.aug_mix(n, size, severity=severity, mixture_width=width, chain_depth=depth, all_ops=all_ops,
                           generator=torch.Generator().manual_seed(5))
        m = n * (1 + width)
        assert list(r["repeat"]) == [j // (1 + width) for j in range(m)]
        assert r["matrices"].shape == (m, 2, 3) and r["matrices"].dtype == np.float32
        assert len(r["tone_ops"]) == len(r["blend"]) == len(r["silent"]) == m
        hi = (severity - 1) / 9.0
        for j in range(m):
            clean = j % (1 + width) == 0
            assert r["silent"][j] == (not clean)  # the chains are silent, the clean frames are not
            tone, mat = r["tone_ops"][j], r["matrices"][j].astype(np.float64)
            if clean:
                assert tone == [] and np.array_equal(mat, np.eye(3)[:2])
                terms = r["blend"][j]
                assert [s for s, _ in terms] == list(range(j, j + 1 + width))
                w = np.array([wt for _, wt in terms], dtype=np.float64)
                assert all(float(np.float32(x)) == x for x in w) and (w >= 0).all()
                assert abs(w.sum() - 1.0) <= (2 + width) * 2.0 ** -24  # each weight and the products rounded once
                continue
            assert r["blend"][j] is None
            assert len(tone) <= (depth if depth > 0 else 3)
            for name, v in tone:
                assert name in names and (all_ops or name in ("posterize", "solarize", "autocontrast", "equalize"))
                if name in ("brightness", "saturation", "contrast", "sharpness"):
                    assert 1.0 - 0.9 * hi - 1e-12 <= v <= 1.0 + 0.9 * hi + 1e-12
                elif name == "posterize":
                    assert v == int(v) and max(4 - round((severity - 1) / 2.25), 1) <= v <= 4
                elif name == "solarize":
                    assert 1.0 - hi - 1e-12 <= v <= 1.0
                else:
                    assert v is None
            # geometry: at most 3 (or depth) of shear <= 0.3 hi, rotate <= 30 hi degrees, translate <= size / 3 hi
            d = depth if depth > 0 else 3
            lin = mat[:, :2]
            assert np.abs(lin - np.eye(2)).max() <= (1.0 + 0.3 * hi) ** d * (1 + np.sin(np.radians(30 * hi))) ** d - 1.0 + 1e-6
            assert np.abs(mat[:, 2]).max() <= d * (max(size) / 3.0 * hi + max(size) * (0.3 * hi + np.sin(np.radians(30 * hi)))) * 2 + 1e-6
    a = decode.aug_mix(6, size, generator=torch.Generator().manual_seed(11))
    b = decode.aug_mix(6, size, generator=torch.Generator().manual_seed(11))
    c = decode.aug_mix(6, size, generator=torch.Generator().manual_seed(12))
    assert np.array_equal(a["matrices"], b["matrices"]) and a["tone_ops"] == b["tone_ops"] and a["blend"] == b["blend"]
    assert not np.array_equal(a["matrices"], c["matrices"]) or a["blend"] != c["blend"]
    # a base matrix is every frame's: the clean frame's own, and what a chain composes onto
    base = np.array([[0.5, 0.0, 10.0], [0.0, 0.5, 20.0]])
    r = decode.aug_mix(3, size, chain_depth=1, generator=torch.Generator().manual_seed(2), base=base)
    assert all(np.array_equal(r["matrices"][j], base.astype(np.float32)) for j in (0, 4, 8))


def test_auto_augment_draws_stay_inside_the_documented_ranges():
    from ccmi import decode
    n = 400
    mats, tones = decode.auto_augment(n, generator=torch.Generator().manual_seed(4), size=(48, 64))
    assert mats.shape == (n, 2, 3) and mats.dtype == np.float32 and len(tones) == n
    seen = set()
    for mat, tone in zip(mats.astype(np.float64), tones):
        assert len(tone) <= 2
        for name, v in tone:
            seen.add(name)
            if name in ("saturation", "contrast", "sharpness"):
                assert 0.1 - 1e-12 <= v <= 1.9 + 1e-12
            elif name == "posterize":
                assert v in (4.0, 5.0, 6.0, 7.0, 8.0)
            elif name == "solarize":
                assert 0.0 <= v <= 1.0
            elif name == "matrix":  # Invert: 1 - x
                assert np.array_equal(np.asarray(v), np.array([[-1, 0, 0, 1], [0, -1, 0, 1], [0, 0, -1, 1]], dtype=np.float64))
            else:
                assert name in ("autocontrast", "equalize") and v is None
        assert np.abs(mat[:, :2] - np.eye(2)).max() <= max(0.3, np.sin(np.radians(30.0))) + 1e-6  # one ShearX or one Rotate
    assert {"equalize", "solarize", "posterize", "saturation", "matrix"} <= seen
    again, tones2 = decode.auto_augment(n, generator=torch.Generator().manual_seed(4), size=(48, 64))
    assert np.array_equal(mats, again) and tones == tones2
    import pytest
    with pytest.raises(ValueError):
        decode.auto_augment(2, policy="cifar10")
