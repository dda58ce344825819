"""tests/colour_ref.py (the float32 restatement of step 3z the GPU tests compare with, bit for bit)
against plain float64 formulas, and the helpers of ccmi.decode that make colour ops: hue_matrix,
grey_matrix, colour_jitter.  No GPU.

The bound between the restatement and the formulas is the project's fp32 parity bound,
2e-5 (1 + max|ref|): an op is at most 7 float32 roundings of values <= 3, and the
fixed-point mean is within 0.5 / 65535 = 7.6e-6 of the float64 mean, times |1 - f| <= 1.5 here."""
import itertools
import math

import numpy as np
import pytest
import torch

import colour_ref as R


def _frame(seed, h=13, w=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3, h, w, generator=g, dtype=torch.float32)


def _close(got, want):
    bound = 2e-5 * (1 + float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    assert err <= bound, (err, bound)


def _ops():
    from ccmi import decode
    return {"brightness": ("brightness", 1.3), "saturation": ("saturation", 0.4), "contrast": ("contrast", 1.7),
            "matrix": ("matrix", decode.hue_matrix(0.07))}


def test_each_op_alone_matches_the_formulas():
    from ccmi import decode
    x = _frame(1)
    for op in (("brightness", 0.0), ("brightness", 0.6), ("brightness", 1.8), ("saturation", 0.0), ("saturation", 1.0),
               ("saturation", 2.5), ("contrast", 0.0), ("contrast", 0.5), ("contrast", 2.5), ("matrix", decode.grey_matrix()),
               ("matrix", decode.hue_matrix(-0.1)), ("matrix", [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]]),
               ("matrix", [[-1, 0, 0, 1], [0, -1, 0, 1], [0, 0, -1, 1]])):
        got = R.apply(x, [op])
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape)
        _close(got, R.apply_f64(x, [op]))
    # exact cases: a permutation moves the channels, brightness 1 and saturation 1 change nothing
    assert torch.equal(R.apply(x, [("matrix", [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]])]), x.flip(0))
    assert torch.equal(R.apply(x, [("brightness", 1.0)]), x)
    assert torch.equal(R.apply(x, [("saturation", 1.0)]), x)
    assert torch.equal(R.apply(x, []), x)


def test_every_order_of_the_four_kinds_matches_the_formulas():
    ops = _ops()
    x = _frame(2)
    seen = set()
    for order in itertools.permutations(sorted(ops)):
        seq = [ops[k] for k in order]
        got = R.apply(x, seq)
        _close(got, R.apply_f64(x, seq))
        seen.add(got.numpy().tobytes())
    assert len(seen) == 24  # the order matters: 24 different frames


def test_the_mean_is_fixed_point():
    x = _frame(3, 7, 9)
    s = R.grey_sum(x)
    g = ((0.2989 * x[0].double() + 0.587 * x[1].double()) + 0.114 * x[2].double()).clamp(0, 1)
    assert abs(s - float((g * 65535).sum())) <= 0.5 * 63 + 1
    m = R.mean_grey(x)
    assert m.dtype == torch.float32 and float(m) == float(np.float32(s / (63 * 65535.0)))
    # a permutation of the pixels does not change the sum, whatever the order of the additions
    p = torch.randperm(63, generator=torch.Generator().manual_seed(4))
    assert R.grey_sum(x.reshape(3, -1)[:, p].reshape(3, 9, 7)) == s
    # all ones: grey = 0.2989 + 0.587 + 0.114 = 0.9999 (the weights do not sum to 1): 65528.4 -> 65528
    one = torch.ones(3, 4, 4)
    assert R.grey_sum(one) == 16 * 65528


def test_hue_matrix():
    from ccmi import decode
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    for h in (0, 1, -1, 2):
        m = decode.hue_matrix(h)
        assert m.dtype == np.float32 and m.shape == (3, 4)
        assert np.abs(m - eye).max() <= 1e-6, h
    for k in range(16):
        h = -0.5 + k / 15.0
        m = decode.hue_matrix(h)
        assert np.all(m[:, 3] == 0)
        for t in (0.0, 0.25, 0.5, 1.0):
            x = torch.full((3, 2, 2), t, dtype=torch.float32)
            assert float((R.apply(x, [("matrix", m)]) - t).abs().max()) <= 1e-6, (h, t)
        # a rotation: h and -h compose to the identity, and luma (row 0 of YIQ) is kept
        back = decode.hue_matrix(-h).astype(np.float64)[:, :3] @ m.astype(np.float64)[:, :3]
        assert np.abs(back - np.eye(3)).max() <= 1e-6
        y = np.array([0.299, 0.587, 0.114])
        assert np.abs(y @ m.astype(np.float64)[:, :3] - y).max() <= 1e-6
    # a quarter turn moves a saturated colour
    red = torch.tensor([1.0, 0.0, 0.0]).reshape(3, 1, 1)
    assert float((R.apply(red, [("matrix", decode.hue_matrix(0.25))]) - red).abs().max()) > 0.3


def test_grey_matrix():
    from ccmi import decode
    m = decode.grey_matrix()
    assert m.dtype == np.float32 and m.shape == (3, 4)
    x = _frame(5)
    got = R.apply(x, [("matrix", m)])
    assert torch.equal(got[0], got[1]) and torch.equal(got[1], got[2])
    assert torch.equal(got[0], R.grey(x).clamp(0, 1))


def test_colour_jitter_ranges_kinds_and_seed():
    from ccmi import decode
    n = 200
    a = decode.colour_jitter(n, 0.4, 0.4, 0.4, 0.1, generator=torch.Generator().manual_seed(7))
    b = decode.colour_jitter(n, 0.4, 0.4, 0.4, 0.1, generator=torch.Generator().manual_seed(7))
    c = decode.colour_jitter(n, 0.4, 0.4, 0.4, 0.1, generator=torch.Generator().manual_seed(8))

    def flat(lists):
        return [(op, np.asarray(v, dtype=np.float64).round(9).tolist()) for f in lists for op, v in f]
    assert flat(a) == flat(b) and flat(a) != flat(c)
    assert len(a) == n
    orders, factors = set(), {"brightness": [], "contrast": [], "saturation": []}
    for ops in a:
        kinds = [op for op, _ in ops]
        assert sorted(kinds) == ["brightness", "contrast", "matrix", "saturation"]  # one op of each kind
        orders.add(tuple(kinds))
        for op, v in ops:
            if op == "matrix":
                # a hue turn within [-0.1, 0.1]: the angle of the (I, Q) rotation, read back through YIQ
                t = np.array(decode._YIQ)
                r = t @ np.asarray(v, np.float64)[:, :3] @ np.linalg.inv(t)
                assert abs(math.atan2(r[2, 1], r[1, 1])) <= 2 * math.pi * 0.1 + 1e-5
                assert np.abs(r[0] - [1, 0, 0]).max() <= 1e-5
            else:
                assert 0.6 <= v <= 1.4
                factors[op].append(v)
    assert len(orders) == 24  # every frame its own order: 200 draws see all of them
    for op, v in factors.items():
        assert min(v) < 0.65 and max(v) > 1.35 and abs(np.mean(v) - 1.0) < 0.06, op
    # an argument of 0 leaves its op out; brightness 1.5 starts at 0; grey_p = 1 ends every frame in grey
    only = decode.colour_jitter(50, brightness=1.5, grey_p=1.0, generator=torch.Generator().manual_seed(1))
    for ops in only:
        assert [op for op, _ in ops] == ["brightness", "matrix"]
        assert 0.0 <= ops[0][1] <= 2.5
        assert np.array_equal(ops[1][1], decode.grey_matrix())
    assert decode.colour_jitter(3) == [[], [], []]
    none = decode.colour_jitter(400, 0.1, grey_p=0.25, generator=torch.Generator().manual_seed(2))
    share = sum(len(ops) == 2 for ops in none) / 400
    assert 0.17 < share < 0.33
    with pytest.raises(ValueError):
        decode.colour_jitter(1, hue=0.6)
    with pytest.raises(ValueError):
        decode.colour_jitter(1, brightness=-0.1)
