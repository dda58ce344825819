"""Reference of the training step's in-kernel quantisation noise (t_quant, csrc/train.hip): a numpy
restatement of the counter-based generator as include/ccmi.h states it (ccmi_train_args.seed), both
transforms in float64, and a-priori bounds for the kernel's float32 evaluation.  A helper: no tests
in it.  tests/test_noise_ref.py pins it on the CPU (inverse, mirror module, distribution,
independence, edges), tests/test_train_noise_gpu.py compares the kernel's draws with it one by one.

Generator.  key = (step << 40) ^ (frame << 32) ^ index, r = mix64(seed ^ mix64(key)),
r2 = mix64(r + 0x632BE59BD9B4E019); u1 = unif(r), u2 = unif(r2), unif(r) = (float32(r >> 40) +
0.5f) * 2^-24 with the add rounded in float32: for r >> 40 >= 2^23 the half is a tie and goes to the
even neighbour, so the upper half of the lattice holds even multiples of 2^-24 only and
r >> 40 = 2^24 - 1 gives u = 1.0 exactly; r >> 40 = 0 gives 2^-25.  `index` is the latent's position
among the frame's N latents, whatever the stride of the latent buffer.  `seed_for` inverts the outer
mix64, so a test can place any r at a counter of its choice.

Transforms, float64, on the float32 values of a and sigma:
  kumaraswamy  b = (2^a (a - 1) + 1) / a,  n = (1 - (1 - u)^(1/b))^(1/a) - 1/2,
               CDF(x) = 1 - (1 - (x + 1/2)^a)^b        (quantizer.py:60-102)
  gaussian     n = sigma sqrt(-2 ln u1) cos(2 pi u2)   (Box-Muller)

Bound 1, Kumaraswamy, in the u domain (`kumaraswamy_tol_u`): |CDF(n_kernel) - u1| <= K(a) 2^-24.
The comparison is made in u because d n / d u is unbounded at both ends for a > 1 while the way
back is well conditioned.  The kernel computes, with kb = fl(1 / b) and ka = fl(1 / a) from the host,
  w = fl(1 - u1); p = exp2(fl(log2(w) kb)); q = fl(1 - p); x = exp2(fl(log2(q) ka)); n = fl(x - 1/2)
and the check computes u' = 1 - (1 - x'^a)^b from x' = n + 1/2 in float64.  Unit: eps = 2^-24, the
relative error of one float32 rounding (half an ulp) and the absolute one for a value below 1.
v_log_f32 and v_exp_f32 are counted at 1 ulp = 2 eps relative: the ROCm installation states no
figure for them, so 1 ulp is an assumption of this bound.  Each error is carried to u with
|du/dp| = b p^(b-1) <= b, |dq'/dx| = a x^(a-1) <= a (a >= 1), and z |ln z| <= 1/e (e = 2.718...)
for the relative error d of an exponent (z^(1+d) - z = z ln z d).  In units of eps:
  first power, u = 1 - p^b, p = w^(1/b)
    fl(1 - u1)                  absolute eps / 2 in w, that is in u directly           1/2
    log2(w), 1 ulp              exponent off by 2 eps: p^b |ln p^b| 2 eps              2 / e
    fl(. * kb)                  exponent off by eps                                    1 / e
    kb itself                   exp2f 1 ulp, then (a - 1), *, + 1, / a, 1 / b in float32:
                                7 eps relative on the exponent                         7 / e
    exp2, 1 ulp                 p off by 2 eps p: b p^b 2 eps                          2 b
  second power, q' = x'^a, u' = 1 - (1 - q')^b
    fl(1 - p)                   absolute eps / 2 in q: b p^(b-1) eps / 2               b / 2
    log2(q), 1 ulp              q |ln q| 2 eps, times b                                2 b / e
    fl(. * ka), ka = fl(1 / a)  exponent off by eps each                               2 b / e
    exp2, 1 ulp                 x off by 2 eps x: q' off by 2 a eps, times b           2 a b
    fl(x - 1/2)                 absolute eps / 2 at most (exact for x >= 1/4)          a b / 2
  K(a) = 1/2 + 10 / e + 5 b / 2 + 4 b / e + 5 a b / 2:  10.7, 16.6, 26.6 for a = 1, 1.5, 2.
At K = 26.6 a draw is still pinned to +-27 of 16.7 M lattice points, and the errors the bound is
there for are thousands of times larger (tests/test_noise_ref.py plants them).  The float32 chain
with log2 / exp2 rounded from float64 (`kumaraswamy_f32`) stays within 1.0, 2.7 and 2.5 eps
(tests/test_noise_ref.py asserts half the bound).
a < 1 is not covered: x^(a-1) is unbounded there, and no preset uses it.

Bound 2, Gaussian, in the value domain (`gaussian_tol`): |n_kernel - n| <= sigma K_g 2^-24 (R + 1),
R = sqrt(-2 ln u1) <= 5.9.  The kernel computes fl(fl(sqrtf(fl(-2 logf(u1))) cospif(fl(2 u2))) sigma);
2 u2 and -2 L are exact.  HIP's math functions are OCML's, written to the OpenCL C specification's
error table, whose figures are used (the ROCm installation carries no table of its own): log <= 3
ulp, sqrt <= 3 ulp, cospi <= 4 ulp; 1 ulp <= 2 eps relative, and <= eps absolute for |cos| <= 1.
In units of eps sigma R:
    logf, 3 ulp, under the square root   R off by 3 eps R        3
    sqrtf, 3 ulp                         R off by 6 eps R        6
    cospif, 4 ulp                        product off by 4 eps R  4
    two products                         2 eps R |cos|           2
  K_g = 15: |n_kernel - n| <= 15 eps sigma R, within the (R + 1) form above.
"""
import math

import numpy as np

E = 2.0 ** -24
_M = (1 << 64) - 1
C_INC = 0x9E3779B97F4A7C15
C_MUL1 = 0xBF58476D1CE4E5B9
C_MUL2 = 0x94D049BB133111EB
C_U2 = 0x632BE59BD9B4E019
C_INV1 = pow(C_MUL1, -1, 1 << 64)
C_INV2 = pow(C_MUL2, -1, 1 << 64)
K_GAUSS = 15.0
R_MAX = math.sqrt(2 * 25 * math.log(2.0))      # u1 = 2^-25: 5.887


def _u64(x):
    if isinstance(x, (int, np.integer)):
        return np.array([int(x) & _M], dtype=np.uint64).reshape(())
    return np.asarray(x).astype(np.uint64)


def _wrap(f, z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        return f(np.atleast_1d(z)).reshape(z.shape)


def mix64(z):
    """The kernel's 64-bit finaliser (splitmix64's), wrapping, on np.uint64."""
    def f(z):
        z = z + np.uint64(C_INC)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(C_MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(C_MUL2)
        return z ^ (z >> np.uint64(31))
    return _wrap(f, z)


def unmix64(z):
    """Inverse of mix64: each xor-shift undone, the inverse multipliers mod 2^64, the increment."""
    def f(z):
        z = z ^ (z >> np.uint64(31)) ^ (z >> np.uint64(62))
        z = z * np.uint64(C_INV2)
        z = z ^ (z >> np.uint64(27)) ^ (z >> np.uint64(54))
        z = z * np.uint64(C_INV1)
        z = z ^ (z >> np.uint64(30)) ^ (z >> np.uint64(60))
        return z - np.uint64(C_INC)
    return _wrap(f, z)


def key(step, b, i):
    return (_u64(step) << np.uint64(40)) ^ (_u64(b) << np.uint64(32)) ^ _u64(i)


def draw_r(seed, step, b, i):
    """(r, r2): the two 64-bit words behind u1 and u2 at counter (seed, step, frame b, index i)."""
    r = mix64(_u64(seed) ^ mix64(key(step, b, i)))
    with np.errstate(over="ignore"):
        r2 = mix64((np.atleast_1d(r) + np.uint64(C_U2)).reshape(r.shape))
    return r, r2


def unif(r):
    """The kernel's 24-bit uniform, its float32 add included; returned as float64."""
    k = (_u64(r) >> np.uint64(40)).astype(np.float32)
    u = (k + np.float32(0.5)) * np.float32(E)
    assert u.dtype == np.float32
    return u.astype(np.float64)


def draw_uniforms(seed, step, b, i):
    r, r2 = draw_r(seed, step, b, i)
    return unif(r), unif(r2)


def seed_for(r, step, b, i):
    """The seed with which the kernel draws exactly r at counter (step, b, i)."""
    return unmix64(r) ^ mix64(key(step, b, i))


def _ab(a):
    a = float(np.float32(a))
    return a, (2.0 ** a * (a - 1.0) + 1.0) / a


def kumaraswamy(u, a):
    a, b = _ab(a)
    u = np.asarray(u, dtype=np.float64)
    return (1.0 - (1.0 - u) ** (1.0 / b)) ** (1.0 / a) - 0.5


def kumaraswamy_cdf(x, a):
    a, b = _ab(a)
    x = np.asarray(x, dtype=np.float64)
    return 1.0 - (1.0 - (x + 0.5) ** a) ** b


def kumaraswamy_pdf(x, a):
    a, b = _ab(a)
    t = np.asarray(x, dtype=np.float64) + 0.5
    return a * b * t ** (a - 1.0) * (1.0 - t ** a) ** (b - 1.0)


def gaussian(u1, u2, sigma):
    s = float(np.float32(sigma))
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    return s * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def gaussian_cdf(x, sigma=1.0):
    x = np.asarray(x, dtype=np.float64) / (float(sigma) * math.sqrt(2.0))
    return 0.5 * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(x))


def kumaraswamy_tol_u(a):
    """Bound 1 of the header: K(a) 2^-24, for a >= 1."""
    a, b = _ab(a)
    assert a >= 1.0, "a < 1 is not covered"
    K = 0.5 + 10.0 / math.e + 2.5 * b + 4.0 * b / math.e + 2.5 * a * b
    return K * E


def gaussian_tol(u1, sigma):
    """Bound 2 of the header, per draw."""
    R = np.sqrt(-2.0 * np.log(np.asarray(u1, dtype=np.float64)))
    return float(np.float32(sigma)) * K_GAUSS * E * (R + 1.0)


def kumaraswamy_f32(u, a):
    """The kernel's float32 chain with log2 / exp2 rounded from float64 (a stand-in for a correctly
    rounded v_log_f32 / v_exp_f32) and the host's float32 1 / a, 1 / b (quant_args)."""
    f = np.float32
    a32 = f(a)
    b32 = (f(np.exp2(np.float64(a32))) * (a32 - f(1)) + f(1)) / a32
    ka, kb = f(1) / a32, f(1) / b32
    lg = lambda v: np.log2(v.astype(np.float64)).astype(f)
    ex = lambda v: np.exp2(v.astype(np.float64)).astype(f)
    with np.errstate(divide="ignore"):
        p = ex(lg(f(1) - np.asarray(u).astype(f)) * kb)
        n = ex(lg(f(1) - p) * ka) - f(0.5)
    assert n.dtype == f
    return n
