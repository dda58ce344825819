"""tests/quant_ref.py on the CPU: the float64 restatement of the step's quantiser agrees with
oracle/train_oracle.py run in float64 wherever the float32 fraction is exact, satisfies the closed
forms of the soft round, and differs from the pure-float64 oracle at T = 1e-4 by exactly the effect
it is there to carry (the fraction formed in float32).

e32_d of the restatement (quantize32 against quantize64, worst input set), as measured where this
file was written: softround_alone and ste 1.4e-7 .. 1.7e-7 at T = 0.3, 0.2, 0.1 and 1.2e-7 at
T = 1e-4 (nobody had measured that one: the float32 tanh holds on the peak of a derivative of
5000 as well as anywhere); softround 1.9e-6 .. 2.9e-6 at T = 0.3 .. 0.1.  The assertion at
T = 0.3 .. 0.1 is 2^-14 = 6.1e-5; at 1e-4 only that the value is finite.  The one entry outside it
is -2^23 under softround (quant_ref.sets_for), pinned here as a fact.
"""
import math

import numpy as np
import pytest
import torch

import quant_ref as Q
import train_oracle as to

TEMPS = (0.3, 0.2, 0.1)


def _oracle64(x32, qtype, T, n32=None):
    """train_oracle.quantize in float64 with autograd, at the float32 value of T: (y, dy/dx)."""
    x = torch.from_numpy(x32.astype(np.float64)).requires_grad_(True)
    n = None if n32 is None else torch.from_numpy(n32.astype(np.float64))
    y = to.quantize(x, qtype, float(np.float32(T)), n)
    y.sum().backward()
    return y.detach().numpy(), x.grad.numpy()


def _exact(x32):
    """Where fl(fl(x - floor(x)) - 0.5) is the exact value."""
    x = x32.astype(np.float64)
    return Q._centred32(x32)[1].astype(np.float64) == x - np.floor(x) - 0.5


def _close(a, b, what):
    # 1e-12 of the largest entry (absolute where that is below 1): numpy's and torch's float64 tanh
    # may differ by a rounding, 1.1e-16, which 1 - th^2 doubles and 0.5 inv / T = 5000 at T = 1e-4
    # carries to 1.1e-12 absolute in a derivative in the tail
    # (the values y are held to 1e-12 of their own size)
    scale = max(1.0, float(np.abs(b).max())) if what[-1] == "d" else np.maximum(1.0, np.abs(b))
    err = np.abs(a - b) / scale
    assert float(err.max()) <= 1e-12, (what, float(err.max()), int(err.argmax()))


MATRIX = [(q, T) for q in Q.QTYPES for T in TEMPS] + [("ste", 1e-4), ("softround_alone", 1e-4)]


@pytest.mark.parametrize("qtype,T", MATRIX)
def test_quantize64_is_the_oracle_in_float64_where_the_fraction_is_exact(qtype, T):
    sets = Q.input_sets(T)
    if qtype == "softround":
        # the restatement rounds y1 and y1 + n to float32, the oracle does not: compared where both
        # are exact, the ties with noise 0, +-1/4, +-1/2
        x, n = sets["ties"]
        y, d = Q.quantize64(x, qtype, T, n)
        yo, do = _oracle64(x, qtype, T, n)
        _close(y, yo, (qtype, T, "y"))
        _close(d, do, (qtype, T, "d"))
        return
    x = np.concatenate([np.abs(sets["randn3"][0]), sets["ties"][0], sets["peak"][0], sets["large"][0]])
    keep = _exact(x)
    assert keep.mean() >= 0.9 and np.all(keep[4096:4096 + 27])          # the dyadic ones are all exact
    x = x[keep]
    assert x.min() < 0 and x.size > 4000
    n = None
    if qtype == "none":
        n = np.random.default_rng(3).uniform(-0.5, 0.5, x.size).astype(np.float32)
    y, d = Q.quantize64(x, qtype, T, n)
    yo, do = _oracle64(x, qtype, T, n)
    _close(y, yo, (qtype, T, "y"))
    _close(d, do, (qtype, T, "d"))
    if qtype in Q.READS_T and T == 1e-4:
        assert d.max() > 4999          # the peak is in the set


@pytest.mark.parametrize("T", TEMPS + (1e-4,))
def test_closed_forms(T):
    T32 = float(np.float32(T))
    inv = Q.inv64(T)
    k = np.arange(-6, 7, dtype=np.float32)
    y, d = Q.quantize64(k, "softround_alone", T)
    assert np.all(np.abs(y - k) <= 1e-15 * np.maximum(1, np.abs(k)))
    y, d = Q.quantize64(k + np.float32(0.5), "softround_alone", T)
    assert np.array_equal(y, k.astype(np.float64) + 0.5)
    assert np.array_equal(d, np.full(k.size, 0.5 / T32 * inv)) and abs(d[0] - inv / (2 * T32)) <= 1e-15 * d[0]
    y, d = Q.quantize64(k, "softround", T, np.zeros(k.size, np.float32))
    assert np.all(np.abs(y - k) <= 1e-15 * np.maximum(1, np.abs(k)))
    for name, (x, n) in Q.input_sets(T).items():
        for qtype in Q.QTYPES:
            y, d = Q.quantize64(x, qtype, T, n)
            assert y.dtype == np.float64 and d.dtype == np.float64
            assert np.all(np.isfinite(y)) and np.all(d >= 0), (name, qtype)
            if qtype == "hardround":
                assert not d.any()
            if qtype in ("true_ste", "none"):
                assert np.all(d == 1)
            if qtype in Q.HARD:
                assert np.array_equal(y, np.rint(x.astype(np.float64)))
            if qtype in Q.READS_T:
                assert d.max() <= (inv / (2 * T32)) ** (2 if qtype == "softround" else 1) * (1 + 1e-15)
    # ties to even
    y, _ = Q.quantize64(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], np.float32), "hardround", T)
    assert y.tolist() == [0, 2, 2, -0.0, -2, -2]
    # noise None is noise 0
    x, n = Q.input_sets(T)["randn3"]
    for qtype in ("none", "softround"):
        a, b = Q.quantize64(x, qtype, T, None), Q.quantize64(x, qtype, T, np.zeros_like(x))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_float32_fraction_matters_at_1e_4_only():
    """x = -0.4999000132 (a float32): x - floor(x) = 0.5000999868 needs one bit more than float32
    has there, so the float32 fraction is 2^-25 off, 3e-4 in the tanh argument at T = 1e-4.  The
    pure-float64 oracle on the same x and the restatement then differ by more than 2^-13 of the
    largest derivative (inv / 2T = 5000); at T = 0.1 by less than 2^-22.  This is why quantize64
    forms the centred fraction in float32, as the kernel and the reference do."""
    x = np.array([-0.4999000132], dtype=np.float32)
    assert not _exact(x)[0]
    for T, lo, hi in ((1e-4, 2.0 ** -13, 2.0 ** -11), (0.1, 0.0, 2.0 ** -22)):
        peak = Q.inv64(T) / (2 * float(np.float32(T)))
        d = Q.quantize64(x, "ste", T)[1][0]
        do = _oracle64(x, "ste", T)[1][0]
        rel = abs(d - do) / peak
        print(f"\nT = {T}: restatement {d:.6g}, pure float64 {do:.6g}, difference 2^{math.log2(rel):.1f} of the peak {peak:.6g}")
        assert lo < rel < hi, (T, d, do, rel)


@pytest.mark.parametrize("qtype", Q.READS_T)
def test_the_restatement_own_float32_distance(qtype):
    for T in TEMPS + (1e-4,):
        worst = (0.0, 0.0, "")
        for name, (x, n) in Q.sets_for(qtype, T).items():
            e_d, e_y = Q.e32(x, qtype, T, n)
            assert math.isfinite(e_d) and math.isfinite(e_y)
            if (qtype, name) == ("softround", "minus2^23"):
                # the one ill-conditioned entry (quant_ref.input_sets): the float32 first stage is 1/2 off
                assert Q.quantize32(x, "softround_alone", T)[0][0] == -2.0 ** 23 + 0.5 and e_y < 2.0 ** -23
                assert e_d > 1 or T == 1e-4      # (at 1e-4 both tails are 0 in float64 too)
                continue
            worst = max(worst, (e_d, e_y, name))
            if T != 1e-4:
                assert e_d <= 2.0 ** -14, (qtype, T, name, e_d)
        print(f"\n{qtype} T = {T}: worst e32_d {worst[0]:.2e} (y {worst[1]:.2e}) on the set {worst[2]}")
