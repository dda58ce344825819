"""tests/msssim_ref.py, the torch restatement of the MS-SSIM distortion (include/ccmi.h), pinned by
closed forms, and the preconditions of the GPU tests' cases, on the CPU.

Measured here (float32 against float64 restatement): e32 between 2^-17.9 and 2^-15.0 on the
MS-SSIM cases (2^-24 for the MSE alone), every v_s at least 0.905, the four outputs within 3.0e-6."""
import math

import pytest
import torch

import msssim_ref as R


def test_taps_sum_to_one_and_are_symmetric():
    g = R.taps()
    assert g.shape == (11,)
    assert abs(float(g.sum()) - 1.0) < 2e-7  # float32 taps, summed in double
    assert torch.equal(g, g.flip(0))
    assert torch.equal(g, g.float().double())  # rounded once to float32
    assert float(g[5]) == float(g.max()) and abs(float(g[4] / g[5]) - math.exp(-1 / 4.5)) < 1e-7


@pytest.mark.parametrize("h,w,S", [(11, 11, 1), (21, 23, 2), (41, 43, 3)])
def test_equal_frames_give_one_and_no_gradient(h, w, S):
    g = torch.Generator().manual_seed(3)
    X = [torch.rand(2, h, w, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3)]
    Y = [x.detach().clone() for x in X]
    out, v = R.evaluate(X, Y, S, R.default_weights(S), (0.25, 0.25, 0.5), 0.0, 1.0)  # weights exact in float32
    assert float((out[:, 1] - 1).abs().max().detach()) < 1e-12 and float((v - 1).abs().max().detach()) < 1e-12
    grads = torch.autograd.grad(out[:, 0].sum(), X)
    assert max(float(gr.abs().max()) for gr in grads) < 1e-12


def test_constant_offset_on_a_flat_plane():
    a, d = 0.4, 0.1
    X = [torch.full((1, 13, 14), a + d, dtype=torch.float64)]
    Y = [torch.full((1, 13, 14), a, dtype=torch.float64)]
    # the float32 taps sum to 1 within 2^-24 a tap: a flat plane's window is the constant within 1e-6
    cs, l = R.scale_terms(X[0], Y[0], R.taps())
    assert float((cs - 1).abs().max()) < 1e-6
    want = (2 * a * (a + d) + R.C1) / (a * a + (a + d) ** 2 + R.C1)
    assert float((l - want).abs().max()) < 1e-6
    out, _ = R.evaluate(X, Y, 1, (1.0,), (1.0,), 1.0, 1.0)
    assert abs(float(out[0, 1]) - want) < 1e-6 and abs(float(out[0, 2]) - d * d) < 1e-12
    assert abs(float(out[0, 0]) - (d * d + 1 - want)) < 1e-6


def test_pooling_matches_an_explicit_loop():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 5, 7, generator=g, dtype=torch.float64)
    y = R.pool(x)
    assert y.shape == (1, 3, 4)
    for i in range(3):
        for j in range(4):
            s = 0.0
            for a in range(2):
                for b in range(2):
                    ii, jj = 2 * i - 1 + a, 2 * j - 1 + b  # 5 and 7 are odd: padding 1 on both axes
                    if 0 <= ii < 5 and 0 <= jj < 7:
                        s += float(x[0, ii, jj])
            assert abs(float(y[0, i, j]) - s / 4) < 1e-15
    assert abs(float(y[0, 0, 0]) - float(x[0, 0, 0]) / 4) < 1e-15  # a padded corner: one sample, divisor 4
    assert R.pool(torch.rand(1, 6, 8, dtype=torch.float64)).shape == (1, 3, 4)
    assert [s for s in R.size_chain(161, 161, 5)] == [(161, 161), (81, 81), (41, 41), (21, 21), (11, 11)]


def test_dead_plane_has_no_ms_gradient():
    g = torch.Generator().manual_seed(7)
    Y = [torch.rand(1, 15, 16, generator=g, dtype=torch.float64) for _ in range(2)]
    X = [(1 - Y[0]).requires_grad_(True), (Y[1] + 0.01).requires_grad_(True)]
    out, v = R.evaluate(X, Y, 1, (1.0,), (0.5, 0.5), 0.0, 1.0)
    assert float(v[0, 0, 0].detach()) < 0 < float(v[0, 1, 0].detach())
    g0, g1 = torch.autograd.grad(out[:, 0].sum(), X)
    assert float(g0.abs().max()) == 0 and float(g1.abs().max()) > 0


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_preconditions(case):
    x, y = R.case_data(case)
    r = R.case_ref(case)
    xs = x[:, r.sampled]
    print(f"\n{case.name}: e32 2^{math.log2(r.e32):.1f}, outputs {r.eout:.2e}, min v_s {float(r.v64.min()):.3f}")
    assert r.e32 <= R.E32_MAX
    assert float(r.v64.min()) >= 0.89  # no relu is hit
    assert float(torch.minimum(xs.abs(), (xs - 1).abs()).min()) >= 1e-4  # no raw value at the clamp's kinks
    if case.H * case.W >= 41 * 43:
        assert bool(((xs < 0) | (xs > 1)).any())  # the clamp mask is exercised
    assert float(r.g64[:, ~r.sampled].abs().max() if (~r.sampled).any() else 0.0) == 0.0
    for h, w in case.sizes:
        assert min(R.size_chain(h, w, case.S)[-1]) >= 11


def test_clamp_mask_is_exercised_somewhere_small_too():
    hit = [c.name for c in R.CASES
           if bool(((R.case_data(c)[0][:, R.case_ref(c).sampled] < 0) | (R.case_data(c)[0][:, R.case_ref(c).sampled] > 1)).any())]
    assert len(hit) >= 8, hit
