"""The bicubic forms of the ccmi_resample and ccmi_warp contracts (include/ccmi.h: CCMI_FILTER_CUBIC,
CCMI_WARP_CUBIC and their clamp flags) in numpy float32, one rounded operation at a time: the
reference of tests/test_decode_cubic_gpu.py and tests/test_decode_cubic_abi.py, pinned by
tests/test_decode_cubic_ref.py against torch's float64 interpolate(bicubic, antialias=True) and
grid_sample(bicubic).  Nothing here calls the library.

The resize weights are integers: np.int64 by Horner, as a kernel would compute them (u_int64), and
Python's unbounded ints by the contract's polynomial as written (u_exact); the ref test holds one
against the other at the contract's extreme sizes."""
import numpy as np

import warp_ref as W

F32 = np.float32
PAD_FILL, PAD_EDGE = W.PAD_FILL, W.PAD_EDGE

# the Keys cubic as integer polynomials in (n, D2), coefficients of n^3, n^2 D2, n D2^2, D2^3 for
# n < D2 and for D2 <= n < 2 D2.  KEYS_HALF is the contract (a = -0.5, times 2); KEYS_075 is a = -0.75
# times 4, which only the ref test's planted error uses.
KEYS_HALF = ((3, -5, 0, 2), (-1, 5, -8, 4))
KEYS_075 = ((5, -9, 0, 4), (-3, 15, -24, 12))


def tap_run(I, O, i):
    """(j0, j1, j0 unclipped, j1 unclipped) of output index i: the j with n(i, j) < 2 D2, clipped to [0, I)."""
    D2, c = 2 * max(I, O), (2 * i + 1) * I
    a, b = c - 2 * D2 - O, c + 2 * D2 - O
    lo, hi = a // (2 * O) + 1, (b - 1) // (2 * O)  # floor division: also right for a < 0
    return max(lo, 0), min(hi, I - 1), lo, hi


def u_exact(n, D2, coef=KEYS_HALF):
    """Python ints, the polynomial as the contract writes it."""
    n, D2 = int(n), int(D2)
    assert 0 <= n < 2 * D2
    k = coef[0] if n < D2 else coef[1]
    return k[0] * n ** 3 + k[1] * n ** 2 * D2 + k[2] * n * D2 ** 2 + k[3] * D2 ** 3


def u_int64(n, D2):
    """np.int64, Horner: ((3 n - 5 D2) n) n + 2 D2^3 and (((5 D2 - n) n - 8 D2^2) n) + 4 D2^3."""
    n, d = np.asarray(n, np.int64), np.int64(D2)
    with np.errstate(over="raise"):
        inner = ((3 * n - 5 * d) * n) * n + 2 * d * d * d
        outer = (((5 * d - n) * n - 8 * d * d) * n) + 4 * d * d * d
    out = np.where(n < d, inner, outer)
    assert out.dtype == np.int64
    return out


def axis_u(I, O, i, coef=KEYS_HALF, renorm=True):
    """(j0, [u(i, j) for the clipped run], U) in Python ints.  renorm=False is the ref test's planted
    error: U summed over the UNCLIPPED run, so the weights of a clipped edge no longer sum to 1."""
    D2, c = 2 * max(I, O), (2 * i + 1) * I
    j0, j1, lo, hi = tap_run(I, O, i)
    us = [u_exact(abs((2 * j + 1) * O - c), D2, coef) for j in range(j0, j1 + 1)]
    U = sum(us) if renorm else sum(u_exact(abs((2 * j + 1) * O - c), D2, coef) for j in range(lo, hi + 1))
    return j0, us, U


def axis_weights(I, O, coef=KEYS_HALF, renorm=True):
    """Per output index: (j0, float32 weights of the taps j0 ..): w = float32(u) / float32(U), the
    conversions from int64 to nearest even, one float32 division."""
    out = []
    for i in range(O):
        j0, us, U = axis_u(I, O, i, coef, renorm)
        assert U > 0 and abs(U) < 2 ** 63 and all(abs(u) < 2 ** 63 for u in us)
        w = np.array(us, np.int64).astype(F32) / np.array(U, np.int64).astype(F32)
        assert w.dtype == F32
        out.append((j0, w))
    return out


def clamp01(r):
    return np.minimum(np.maximum(r, F32(0)), F32(1))


def resample(q, oh, ow, clamp=False, coef=KEYS_HALF, renorm=True):
    """q: [C, h, w] float32 -> [C, oh, ow] float32: steps 3b-3c with the cubic weights, each sum from
    0 over the taps ascending, every product and sum one float32 operation; then the optional clamp."""
    q = np.ascontiguousarray(q)
    assert q.dtype == F32 and q.ndim == 3
    C, h, w = q.shape
    t = np.zeros((C, h, ow), F32)
    for i, (j0, ws) in enumerate(axis_weights(w, ow, coef, renorm)):
        acc = np.zeros((C, h), F32)
        for k, wk in enumerate(ws):
            acc = acc + wk * q[:, :, j0 + k]
            assert acc.dtype == F32
        t[:, :, i] = acc
    r = np.zeros((C, oh, ow), F32)
    for i, (j0, ws) in enumerate(axis_weights(h, oh, coef, renorm)):
        acc = np.zeros((C, ow), F32)
        for k, wk in enumerate(ws):
            acc = acc + wk * t[:, j0 + k, :]
            assert acc.dtype == F32
        r[:, i, :] = acc
    return clamp01(r) if clamp else r


def coefficients(f, A=-0.75):
    """Step 3d's four coefficients of a fraction f (an array of float32 or float64), in its dtype."""
    dt = f.dtype.type
    A, one = dt(A), dt(1)
    A2, A3, A5, A8, A4 = A + dt(2), A + dt(3), dt(5) * A, dt(8) * A, dt(4) * A  # exact for A = -0.75 and -0.5

    def c_in(t):
        return (((A2 * t) - A3) * t) * t + one

    def c_out(s):
        return ((((A * s) - A5) * s + A8) * s) - A4
    g = one - f
    out = [c_out(f + one), c_in(f), c_in(g), c_out(g + one)]
    assert all(c.dtype == f.dtype for c in out)
    return out


def warp(q, m, oh, ow, pad=PAD_FILL, fill=(0.0, 0.0, 0.0), clamp=False, dtype=F32, A=-0.75):
    """q: [3, H, W] over the whole frame -> r' [3, oh, ow]: steps 3a-3b of ccmi_warp (warp_ref.positions),
    then the 16 taps and the two sums of CCMI_WARP_CUBIC, every operation one of `dtype`."""
    q = np.ascontiguousarray(q).astype(dtype)
    C, H, Wd = q.shape
    x0, fx, y0, fy = W.positions(m, oh, ow, dtype)
    fillv = np.asarray(fill, F32).reshape(-1).astype(dtype)
    if fillv.size == 1:
        fillv = np.repeat(fillv, C)

    def tap(a, b):
        yy, xx = y0 - 1 + a, x0 - 1 + b
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < Wd)
        t = q[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, Wd - 1)]
        if pad == PAD_FILL:
            t = np.where(inside[None], t, fillv[:, None, None])
        else:
            assert pad == PAD_EDGE
        return t.astype(dtype)
    wx, wy = coefficients(fx, A), coefficients(fy, A)
    r = np.zeros((C, oh, ow), dtype)
    for a in range(4):
        row = np.zeros((C, oh, ow), dtype)
        for b in range(4):
            row = row + tap(a, b) * wx[b]
        r = r + row * wy[a]
    assert r.dtype == dtype
    if clamp:
        r = np.minimum(np.maximum(r, dtype(0)), dtype(1))
    return r


def taps_in_frame(m, oh, ow, H, Wd):
    """(ys, xs) of every one of the 16 taps per pixel that lies in the frame (what a window must hold)."""
    x0, _, y0, _ = W.positions(m, oh, ow)
    ys = np.concatenate([(y0 - 1 + a).ravel() for a in range(4) for _ in range(4)])
    xs = np.concatenate([(x0 - 1 + b).ravel() for _ in range(4) for b in range(4)])
    ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < Wd)
    return ys[ok], xs[ok]


def window(m, oh, ow, H, Wd, even=False, reach=2):
    """The plan's window (x, y, w, h): warp_ref.window's rule with the cubic's reach, columns
    floor(min xs - 0.5) - 2 .. floor(max xs - 0.5) + 3 and rows alike (reach=1: the bilinear rule)."""
    m = np.asarray(m, F32).reshape(6).astype(np.float64)
    ends = []
    for r, n in ((0, Wd), (1, H)):
        v = [m[3 * r] * cx + m[3 * r + 1] * cy + m[3 * r + 2] for cx in (0.5, ow - 0.5) for cy in (0.5, oh - 0.5)]
        lo = int(min(max(np.floor(min(v) - 0.5) - reach, 0), n - 1))
        hi = int(min(max(np.floor(max(v) - 0.5) + reach + 1, 0), n - 1)) + 1
        if even:
            lo, hi = lo & ~1, (hi + 1) & ~1
        ends.append((lo, hi))
    (xa, xb), (ya, yb) = ends
    return xa, ya, xb - xa, yb - ya
