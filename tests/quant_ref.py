"""The quantiser of the training step (t_quant in train.hip, behind ccmi_quantize_f32 and the mirror
quantize()) restated in float64.  A helper: no tests in it.  tests/test_quant_ref.py pins it on the
CPU, tests/test_softround_gpu.py and tests/test_train_schedule_gpu.py compare the kernel with it.

quantize64(x32, qtype, T, noise32=None) -> (y64, d64), the six types of ccmi_train_args.quantizer
at gain = 1 (the step multiplies x by the gain before and d by the gain after: dq = gain * d):
    T32 = float32(T), and inv = 1 / tanh(1 / (2 T32)) in float64 from T32
    softround s(x):  fx = floor(x) and the centred fraction c = fl(fl(x - fx) - 0.5) in float32, as
                     the kernel (and the reference's float32 run) forms them; then in float64
                     th = tanh(c / T32),  s = fx + 0.5 th inv + 0.5,  s' = 0.5 (1 - th^2) / T32 inv
    none             y = x + n              d = 1
    softround_alone  y = s(x)               d = s'(x)
    softround        y = s(fl(y1 + n))      d = s'(fl(y1 + n)) s'(x),  y1 = float32(s(x)): the second
                     stage's input is the float32 sum of the first stage's float32 value and n
    ste              y = rint(x)            d = s'(x)
    true_ste         y = rint(x)            d = 1
    hardround        y = rint(x)            d = 0        (rint: ties to even, as rintf and torch.round)
Why c in float32: x - floor(x) is not exact for negative x (x = -0.4999 needs one bit more than x
has after the subtraction of -1), so c carries up to 2^-25 of absolute error, 2.5e-4 in the tanh
argument at T = 1e-4.  The kernel uses the reference's own expression, so a float64 restatement
has to start from the same float32 c (tests/test_quant_ref.py pins the size of the effect).

quantize32 runs the same sequence with every operation rounded to float32 (numpy); its distance
from quantize64 is the restatement's own float32 error:
    e32_d = max |d32 - d64| / max |d64|         e32_y = max (|y32 - y64| / max(1, |y64|))
Bounds (`bounds`), the convention of tests/train_ref.py:
    |d_gpu - d64| <= 16 max(e32_d, 2^-22) max |d64|              at every entry
    |y_gpu - y64| <= 16 max(e32_y, 2^-22) max(1, |y64|)          at every entry, |y64| its own
The factor 16 is the one train_ref.py chose before any kernel was run against it.  The floor
2^-22 is there because quantize32 can land on the float64 value exactly (the trivial types, or a
set made of ties only), and the kernel may still differ from numpy's float32 by a few roundings
(its tanhf, and inv rounded to float on the host).  For none, true_ste and hardround no
transcendental is involved: the tests assert d equal and y within one rounding (rint exact).

Input sets (`input_sets`), seeded, a few thousand values at most each; see the function.
"""
import numpy as np

QTYPES = ("none", "softround_alone", "softround", "hardround", "ste", "true_ste")
READS_T = ("softround_alone", "softround", "ste")
HARD = ("hardround", "ste", "true_ste")      # y = rint(x)
TRIVIAL = ("none", "true_ste", "hardround")  # no transcendental
FACTOR = 16.0
FLOOR = 2.0 ** -22
F32 = np.float32


def _centred32(x32):
    """(floor(x), fl(fl(x - floor(x)) - 0.5)), both float32."""
    assert x32.dtype == np.float32
    fx = np.floor(x32)
    c = (x32 - fx) - F32(0.5)
    assert fx.dtype == np.float32 and c.dtype == np.float32
    return fx, c


def inv64(T):
    T32 = float(F32(T))
    return 1.0 / np.tanh(1.0 / (2.0 * T32))


def _soft64(x32, T):
    T32 = float(F32(T))
    inv = inv64(T)
    fx, c = _centred32(x32)
    th = np.tanh(c.astype(np.float64) / T32)
    return fx.astype(np.float64) + 0.5 * th * inv + 0.5, 0.5 * (1.0 - th * th) / T32 * inv


def _soft32(x32, T):
    T32 = F32(T)
    inv = F32(1) / np.tanh(F32(1) / (F32(2) * T32))
    fx, c = _centred32(x32)
    th = np.tanh(c / T32)
    y = fx + F32(0.5) * th * inv + F32(0.5)
    d = F32(0.5) * (F32(1) - th * th) / T32 * inv
    assert y.dtype == np.float32 and d.dtype == np.float32
    return y, d


def _quantize(x32, qtype, T, noise32, soft, dt):
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    n32 = None if noise32 is None else np.ascontiguousarray(noise32, dtype=np.float32)
    x = x32.astype(dt)
    one, zero = np.ones(x32.shape, dt), np.zeros(x32.shape, dt)
    if qtype == "none":
        return (x if n32 is None else x + n32.astype(dt)), one
    if qtype == "softround_alone":
        return soft(x32, T)
    if qtype == "softround":
        y1, dx = soft(x32, T)
        z = y1.astype(np.float32)
        if n32 is not None:
            z = z + n32
        y, du = soft(z, T)
        return y, du * dx
    y = np.rint(x32).astype(dt)
    if qtype == "ste":
        return y, soft(x32, T)[1]
    if qtype == "true_ste":
        return y, one
    if qtype == "hardround":
        return y, zero
    raise ValueError(qtype)


def quantize64(x32, qtype, T, noise32=None):
    """(y, dy/dx) of the header, float64 arrays, from float32 x (and noise)."""
    return _quantize(x32, qtype, T, noise32, _soft64, np.float64)


def quantize32(x32, qtype, T, noise32=None):
    """The same sequence with every operation rounded to float32; float32 arrays."""
    return _quantize(x32, qtype, T, noise32, _soft32, np.float32)


def e32(x32, qtype, T, noise32=None):
    """(e32_d, e32_y) of the header (0 for d where max |d64| = 0: hardround)."""
    y64, d64 = quantize64(x32, qtype, T, noise32)
    y32, d32 = quantize32(x32, qtype, T, noise32)
    dmax = float(np.abs(d64).max())
    e_d = float(np.abs(d32.astype(np.float64) - d64).max()) / dmax if dmax > 0 else 0.0
    e_y = float((np.abs(y32.astype(np.float64) - y64) / np.maximum(1.0, np.abs(y64))).max())
    return e_d, e_y


def bounds(x32, qtype, T, noise32=None):
    """(y64, d64, per-entry bound on y, bound on d (a scalar), e32_y, e32_d)."""
    y64, d64 = quantize64(x32, qtype, T, noise32)
    e_d, e_y = e32(x32, qtype, T, noise32)
    by = FACTOR * max(e_y, FLOOR) * np.maximum(1.0, np.abs(y64))
    bd = FACTOR * max(e_d, FLOOR) * float(np.abs(d64).max())
    return y64, d64, by, bd, e_y, e_d


def input_sets(T, seed=0):
    """name -> (x, n): float32 inputs and a noise array for them (what `none` and `softround` add;
    the other types ignore it).
      randn3     3 randn(4096), the set of tests/test_mirror_train_gpu.py; noise uniform in (-1/2, 1/2)
      ties       every integer and half-integer of [-6, 6] (ties of rintf / torch.round at a fraction of
                 0 and of 1/2 exactly) and +-0.0; noise 0, +-1/4 and +-1/2 in turn
      near       2^-24 either side of the integers and of the halves of (-1, 0) and (0, 1)
      peak       k + 1/2 + j T / 2, j = -20 .. 20, k = -3 .. 3: the derivative's peak and both tails at
                 every T
      large      +-2^10, 2^20, 2^23 - 1/2, 2^23, 2^24 (from 2^23 on the fraction is 0 and y = x)
      crossing   (softround only: `sets_for`) noise that carries y1 + n onto an integer exactly, 2^-20
                 either side of it, and onto the halves next to it (the peak), y1 the float32 first stage of 3 randn(512) at this T
    """
    g = np.random.default_rng(1000 + seed)
    f = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
    sets = {}
    x = f(3.0 * g.standard_normal(4096))
    sets["randn3"] = (x, f(g.uniform(-0.5, 0.5, x.size)))
    x = np.concatenate([f(np.arange(-12, 13) / 2.0), np.array([0.0, -0.0], dtype=np.float32)])
    x = np.tile(x, 5)
    sets["ties"] = (x, f(np.repeat([0.0, 0.25, -0.25, 0.5, -0.5], x.size // 5)))
    u = 2.0 ** -24
    near = [u, 0.5 - u, 0.5 + u, 1.0 - u]
    x = f(near + [-v for v in near])
    assert np.all(x.astype(np.float64) == np.array(near + [-v for v in near]))   # all representable
    sets["near"] = (x, f(g.uniform(-0.5, 0.5, x.size)))
    T32 = float(np.float32(T))
    x = f([k + 0.5 + j * T32 / 2 for k in range(-3, 4) for j in range(-20, 21)])
    sets["peak"] = (x, f(g.uniform(-0.5, 0.5, x.size)))
    mags = [2.0 ** 10, 2.0 ** 20, 2.0 ** 23 - 0.5, 2.0 ** 23, 2.0 ** 24]
    x = f(mags + [-v for v in mags])
    assert np.all(x.astype(np.float64) == np.array(mags + [-v for v in mags]))
    sets["large"] = (x, f(g.uniform(-0.5, 0.5, x.size)))
    x = np.repeat(f(3.0 * g.standard_normal(512)), 8)
    y1 = _soft64(x, T)[0].astype(np.float32)
    k = np.floor(y1) + np.tile(np.array([0, 0, 0, 1, 1, 1, 0.5, -0.5], dtype=np.float32), 512)
    n = (k - y1) + np.tile(np.array([0, 2.0 ** -20, -2.0 ** -20] * 2 + [0, 0], dtype=np.float32), 512)
    assert n.dtype == np.float32
    z = (y1 + n).reshape(512, 8)
    assert np.mean(z[:, [0, 3]] == np.rint(z[:, [0, 3]])) > 0.9   # onto the integer where k - y1 is exact
    sets["crossing"] = (x, n)
    return sets


def sets_for(qtype, T, seed=0):
    """The input sets a type is checked on: those of input_sets, but
      crossing   for softround only (its x are 3 randn, which randn3 has already; the set is about
                 the noise)
      minus2^23  for softround, -2^23 is taken out of `large` into a set of its own.  In float32 the
                 soft round's sum fx + 0.5 th inv + 0.5 does not return x there: 0.5 th inv is
                 -0.49999997, -2^23 - 0.49999997 rounds to -2^23 (the spacing is 1 below it) and
                 + 0.5 gives -2^23 + 1/2, which is representable.  That is 6e-8 of y, but softround's
                 second stage then sits on its peak instead of in its tail: e32_d is above 1 on
                 this one entry and its bound on d says nothing.  A set of its own so that it does
                 not loosen the bound of the others."""
    sets = input_sets(T, seed)
    if qtype != "softround":
        del sets["crossing"]
        return sets
    x, n = sets["large"]
    keep = x != -2.0 ** 23
    sets["large"] = (x[keep], n[keep])
    sets["minus2^23"] = (x[~keep], n[~keep])
    assert sets["minus2^23"][0].size == 1
    return sets
