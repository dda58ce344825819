"""The reference of the in-kernel quantisation noise (tests/noise_ref.py) pinned on the CPU: the
inverse of mix64, constructed draws, the Kumaraswamy formula against the mirror module, and the
generator's design -- distribution, independence across every part of the key, the two edge values
of the 24-bit uniform -- asserted on the restatement, where the inputs are fixed and the outcome is
deterministic.  tests/test_train_noise_gpu.py ties the kernel to this restatement draw by draw; who
changes the key mixing in t_quant changes noise_ref.py and faces these tests.

On these inputs (seeds 0, 1, 2^63 + 5; steps 1, 2, 10600; frames 0, 1, 2; indices 0 .. 16383):
sqrt(n) KS is 0.52 .. 0.99 against the 1.95 asserted, the Gaussian mean at most 0.8 / sqrt(n), its
standard deviation at most 1.0 / sqrt(2 n) off 1, the largest correlation 3.55 / sqrt(N).
"""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import noise_ref as R

SEEDS = (0, 1, 2 ** 63 + 5)
STEPS = (1, 2, 10600)
FRAMES = (0, 1, 2)
N = 16384
PARAMS = (1.0, 1.5, 2.0)
STREAMS = list(itertools.product(STEPS, FRAMES))


@functools.lru_cache(maxsize=None)
def _streams(seed):
    """{(step, frame): (u1, u2)} of one seed, read-only."""
    out = {}
    for step, b in STREAMS:
        u1, u2 = R.draw_uniforms(seed, step, b, np.arange(N))
        u1.setflags(write=False)
        u2.setflags(write=False)
        out[step, b] = (u1, u2)
    return out


def _pooled(seed):
    s = _streams(seed)
    return np.concatenate([s[k][0] for k in STREAMS]), np.concatenate([s[k][1] for k in STREAMS])


def _ks(x, cdf):
    x = np.sort(x)
    F, n = cdf(x), x.size
    return max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n))


def _corr(x, y):
    x, y = x - x.mean(), y - y.mean()
    return float(x @ y / math.sqrt((x @ x) * (y @ y)))


def test_unmix64_inverts_mix64():
    rng = np.random.default_rng(0)
    z = rng.integers(0, 2 ** 64, size=1000, dtype=np.uint64)
    assert np.array_equal(R.unmix64(R.mix64(z)), z)
    assert np.array_equal(R.mix64(R.unmix64(z)), z)
    # splitmix64's first output for state 0 (the published test vector of the finaliser)
    assert int(R.mix64(0)) == 0xE220A8397B1DCDAF


def test_seed_for_constructs_the_draw():
    rng = np.random.default_rng(1)
    r = rng.integers(0, 2 ** 64, size=64, dtype=np.uint64)
    step, b, i = 3, 1, np.arange(64) * 37
    seeds = R.seed_for(r, step, b, i)
    for k in range(64):
        got, _ = R.draw_r(int(seeds[k]), step, b, int(i[k]))
        assert int(got) == int(r[k])


@pytest.mark.parametrize("a", PARAMS)
def test_kumaraswamy_formula_is_the_mirror_modules(a):
    from coolchic.enc.component.core.quantizer import generate_kumaraswamy_noise
    u = np.linspace(0.0, 1.0, 4097)[1:-1]
    ref = generate_kumaraswamy_noise(torch.from_numpy(u), a).numpy()
    assert ref.dtype == np.float64
    n = R.kumaraswamy(u, a)
    assert np.max(np.abs(n - ref)) <= 1e-15
    if a == 1.0:
        assert np.max(np.abs(n - (u - 0.5))) <= 1e-15
    assert np.max(np.abs(R.kumaraswamy_cdf(n, a) - u)) <= 1e-12
    if a > 1.0:
        x = np.linspace(-0.5, 0.5, 100001)
        assert abs(x[np.argmax(R.kumaraswamy_pdf(x, a))]) <= 2e-5      # the mode of the density at 0


@pytest.mark.parametrize("seed", SEEDS)
def test_distribution(seed):
    u1, u2 = _pooled(seed)
    n = u1.size
    assert n == 9 * N
    bound = 1.95 / math.sqrt(n)                                        # the Kolmogorov 0.1 % point
    for a in PARAMS:
        ks = _ks(R.kumaraswamy(u1, a), lambda x: R.kumaraswamy_cdf(x, a))
        print(f"seed {seed} kumaraswamy {a}: sqrt(n) KS {ks * math.sqrt(n):.3f}")
        assert ks <= bound, (a, ks * math.sqrt(n))
    g = R.gaussian(u1, u2, 1.0)
    ks = _ks(g, R.gaussian_cdf)
    print(f"seed {seed} gaussian: sqrt(n) KS {ks * math.sqrt(n):.3f}, mean {g.mean() * math.sqrt(n):.3f} / sqrt(n), "
          f"std - 1 {(g.std() - 1) * math.sqrt(2 * n):.3f} / sqrt(2n)")
    assert ks <= bound, ks * math.sqrt(n)
    assert abs(g.mean()) <= 4 / math.sqrt(n)
    assert abs(g.std() - 1.0) <= 4 / math.sqrt(2 * n)


@pytest.mark.parametrize("seed", SEEDS)
def test_independence_within_a_seed(seed):
    s = _streams(seed)
    bound, worst = 5 / math.sqrt(N), 0.0
    gs = {k: R.gaussian(*s[k], 1.0) for k in STREAMS}
    for k1, k2 in itertools.combinations(STREAMS, 2):                  # across steps and frames
        for c in (_corr(s[k1][0], s[k2][0]), _corr(gs[k1], gs[k2])):
            worst = max(worst, abs(c))
            assert abs(c) <= bound, (k1, k2, c * math.sqrt(N))
    for k in STREAMS:
        for lag in (1, 2, 64, 256):                                     # along the index
            for x in (s[k][0], gs[k]):
                c = _corr(x[:-lag], x[lag:])
                worst = max(worst, abs(c))
                assert abs(c) <= bound, (k, lag, c * math.sqrt(N))
        c = _corr(s[k][0], s[k][1])                                     # u1 against u2 of the same counter
        worst = max(worst, abs(c))
        assert abs(c) <= bound, (k, "u1 u2", c * math.sqrt(N))
    print(f"seed {seed}: largest |correlation| {worst * math.sqrt(N):.2f} / sqrt(N)")


def test_independence_across_seeds():
    for s1, s2 in itertools.combinations(SEEDS, 2):
        a, b = _streams(s1)[1, 0], _streams(s2)[1, 0]
        for c in (_corr(a[0], b[0]), _corr(R.gaussian(*a, 1.0), R.gaussian(*b, 1.0))):
            assert abs(c) <= 5 / math.sqrt(N), (s1, s2, c * math.sqrt(N))


def test_edges_of_the_uniform():
    top, bottom = (2 ** 24 - 1) << 40, (1 << 40) - 1                   # r >> 40 = 2^24 - 1 and 0
    assert float(R.unif(top)) == 1.0 and float(R.unif(bottom)) == 2.0 ** -25
    assert float(R.unif((2 ** 23 + 1) << 40)) == (2 ** 23 + 2) * 2.0 ** -24   # the tie goes to the even neighbour
    assert float(R.unif((2 ** 23 - 1) << 40)) == (2 ** 23 - 0.5) * 2.0 ** -24   # below 2^23 the half is kept
    for a in PARAMS:
        hi, lo = float(R.kumaraswamy(1.0, a)), float(R.kumaraswamy(2.0 ** -25, a))
        assert hi == 0.5 and -0.5 <= lo < -0.499
        f = R.kumaraswamy_f32(np.array([1.0, 2.0 ** -25]), a)          # the float32 chain: +1/2 and -1/2
        assert f[0] == np.float32(0.5) and f[1] == np.float32(-0.5)
    for sigma in (0.25, 0.1):
        for u2 in (2.0 ** -25, 0.25, 1.0):
            assert float(R.gaussian(1.0, u2, sigma)) == 0.0
            g = float(R.gaussian(2.0 ** -25, u2, sigma))
            assert math.isfinite(g) and abs(g) <= 5.9 * sigma
    assert R.R_MAX <= 5.9


@pytest.mark.parametrize("a", PARAMS)
def test_float32_chain_meets_the_u_domain_bound(a):
    """The kernel's operations in numpy float32, log2 / exp2 rounded from float64: the a-priori
    bound must hold for it with room (the ulp of the device's log2 / exp2 comes on top)."""
    u1, _ = _pooled(0)
    err = np.abs(R.kumaraswamy_cdf(R.kumaraswamy_f32(u1, a), a) - u1)
    print(f"a = {a}: worst {err.max() / R.E:.2f} x 2^-24 of the {R.kumaraswamy_tol_u(a) / R.E:.1f} allowed")
    assert err.max() <= 0.5 * R.kumaraswamy_tol_u(a)


def test_wrong_formulas_are_far_outside_the_bounds():
    """What the bounds are for: b without the / a, 1/a and 1/b swapped, a lost - 1/2, sigma twice,
    u2 taken from r, index bits shifted into the frame's -- each is off by orders of magnitude."""
    u1, u2 = (x[:N] for x in _pooled(1))
    a, (af, b) = 2.0, R._ab(2.0)
    tol = R.kumaraswamy_tol_u(a)
    wrong = {
        "b without / a": (1 - (1 - u1) ** (1 / (b * af))) ** (1 / af) - 0.5,
        "1/a and 1/b swapped": (1 - (1 - u1) ** (1 / af)) ** (1 / b) - 0.5,
        "lost - 1/2": (1 - (1 - u1) ** (1 / b)) ** (1 / af),
        "another index": R.kumaraswamy(R.draw_uniforms(1, 1, 0, np.arange(N) + 1)[0], a),
    }
    for name, n in wrong.items():
        with np.errstate(invalid="ignore"):
            err = np.abs(R.kumaraswamy_cdf(n, a) - u1)
        assert not np.all(err <= tol) and np.nanmedian(err) > 1000 * tol, name
    g, gt = R.gaussian(u1, u2, 0.25), R.gaussian_tol(u1, 0.25)
    for name, n in {"sigma twice": 0.25 * g, "u2 from r": R.gaussian(u1, u1, 0.25)}.items():
        assert np.median(np.abs(n - g) / gt) > 1000, name
