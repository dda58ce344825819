"""Step 3a' of the ccmi_warp contract with CCMI_WARP_PROJECTIVE (include/ccmi.h) in numpy float32, one
rounded operation at a time, the plan's check quantities S_r, D, D', E_r and its window rule: the
reference of tests/test_decode_persp_gpu.py and tests/test_decode_persp_abi.py, pinned by
tests/test_decode_persp_ref.py against torch's grid_sample in float64.  Nothing here calls the library.

The tap steps 3b-3d are those of tests/warp_ref.py and tests/cubic_ref.py, imported and not restated:
both take their positions from warp_ref.positions, which warp() / cubic() below replace with the
projective positions for the length of the call."""
import contextlib

import numpy as np

import cubic_ref as R
import warp_ref as W

F32 = np.float32
PAD_FILL, PAD_EDGE = W.PAD_FILL, W.PAD_EDGE
WARP_CUBIC, WARP_CLAMP, WARP_PROJECTIVE = 0x100, 0x200, 0x800
EPS = 2.0 ** -24
MAX_REACH = 2.0 ** 22
MAX_E = 0.875


def as9(m6):
    """The 6-entry matrix with the row 0 0 1 appended."""
    return np.concatenate([np.asarray(m6, F32).reshape(6), np.asarray([0, 0, 1], F32)])


def source(m, oh, ow, dtype=F32):
    """Step 3a': (xs, ys), each [oh, ow], of every output pixel.  m: the nine entries.  float32 is the
    contract (numpy's float32 division is the correctly rounded IEEE quotient), float64 the definition."""
    m = np.asarray(m, F32).reshape(9).astype(dtype)
    half = dtype(0.5)
    cx = (np.arange(ow).astype(dtype) + half)[None, :]
    cy = (np.arange(oh).astype(dtype) + half)[:, None]
    xn = ((m[0] * cx) + (m[1] * cy)) + m[2]
    yn = ((m[3] * cx) + (m[4] * cy)) + m[5]
    wn = ((m[6] * cx) + (m[7] * cy)) + m[8]
    assert xn.dtype == dtype and yn.dtype == dtype and wn.dtype == dtype and wn.shape == (oh, ow)
    xs, ys = xn / wn, yn / wn
    assert xs.dtype == dtype and ys.dtype == dtype
    return xs, ys


def positions(m, oh, ow, dtype=F32):
    """Steps 3a'-3b: (x0, fx, y0, fy) as warp_ref.positions returns them."""
    xs, ys = source(m, oh, ow, dtype)
    half = dtype(0.5)
    u, v = xs - half, ys - half
    x0f, y0f = np.floor(u), np.floor(v)
    fx, fy = u - x0f, v - y0f
    assert fx.dtype == dtype
    return x0f.astype(np.int64), fx, y0f.astype(np.int64), fy


@contextlib.contextmanager
def _projective(m9):
    """warp_ref.positions gives the projective positions of m9 while the block runs."""
    saved = W.positions
    W.positions = lambda _m, oh, ow, dtype=F32: positions(m9, oh, ow, dtype)
    try:
        yield
    finally:
        W.positions = saved


def warp(q, m, oh, ow, pad=PAD_FILL, fill=(0.0, 0.0, 0.0), dtype=F32):
    """warp_ref.warp (the four bilinear taps) at the projective positions of the nine entries m."""
    with _projective(m):
        return W.warp(q, np.zeros(6, F32), oh, ow, pad, fill, dtype)


def cubic(q, m, oh, ow, pad=PAD_FILL, fill=(0.0, 0.0, 0.0), clamp=False, dtype=F32):
    """cubic_ref.warp (the sixteen taps) at the projective positions of the nine entries m."""
    with _projective(m):
        return R.warp(q, np.zeros(6, F32), oh, ow, pad, fill, clamp, dtype)


def render(q, m, oh, ow, pad_word, fill=(0.0, 0.0, 0.0), dtype=F32):
    """r' for a whole ccmi_warp.pad word with CCMI_WARP_PROJECTIVE set."""
    assert pad_word & WARP_PROJECTIVE
    if pad_word & WARP_CUBIC:
        return cubic(q, m, oh, ow, pad_word & 1, fill, bool(pad_word & WARP_CLAMP), dtype)
    return warp(q, m, oh, ow, pad_word & 1, fill, dtype)


def taps_in_frame(m, oh, ow, H, Wd, reach=1):
    """(ys, xs) of every tap of the float32 contract that lies in the frame (reach 1: the 4 bilinear
    taps, 2: the cubic's 16)."""
    x0, _, y0, _ = positions(m, oh, ow)
    offs = range(0, 2) if reach == 1 else range(-1, 3)
    ys = np.concatenate([(y0 + a).ravel() for a in offs for _ in offs])
    xs = np.concatenate([(x0 + b).ravel() for _ in offs for b in offs])
    ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < Wd)
    return ys[ok], xs[ok]


def quantities(m, oh, ow, H, Wd):
    """The plan's check quantities in float64 from the float32 entries: S (three), D, Dp, E (two; inf
    where Dp <= 0)."""
    m = np.asarray(m, F32).reshape(9).astype(np.float64)
    S = [abs(m[3 * r]) * ow + abs(m[3 * r + 1]) * oh + abs(m[3 * r + 2]) for r in range(3)]
    D = min(m[6] * cx + m[7] * cy + m[8] for cx in (0.5, ow - 0.5) for cy in (0.5, oh - 0.5))
    Dp = D - 3 * EPS * S[2]
    E = [3 * EPS * (S[r] + (L + 3) * S[2]) / Dp + 2 * EPS * (L + 3) if Dp > 0 else np.inf for r, L in ((0, Wd), (1, H))]
    return {"S": S, "D": D, "Dp": Dp, "E": E}


def refusal(m, oh, ow, H, Wd):
    """None if the plan accepts the matrix, else a word of its message."""
    if not np.isfinite(np.asarray(m, F32)).all():
        return "finite"
    c = quantities(m, oh, ow, H, Wd)
    if max(c["S"]) > MAX_REACH:
        return "2^22"
    if not c["Dp"] > 0:
        return "denominator"
    if max(c["S"][0], c["S"][1]) / c["Dp"] > MAX_REACH:
        return "2^22"
    if max(c["E"]) > MAX_E:
        return "too strong"
    return None


def window(m, oh, ow, H, Wd, even=False, reach=1):
    """The plan's window (x, y, w, h): warp_ref.window's rule on the quotients at the four corner pixel
    centres, in float64 from the float32 entries (reach 2: the cubic's)."""
    m = np.asarray(m, F32).reshape(9).astype(np.float64)
    ends = []
    for r, n in ((0, Wd), (1, H)):
        v = [(m[3 * r] * cx + m[3 * r + 1] * cy + m[3 * r + 2]) / (m[6] * cx + m[7] * cy + m[8])
             for cx in (0.5, ow - 0.5) for cy in (0.5, oh - 0.5)]
        lo = int(min(max(np.floor(min(v) - 0.5) - reach, 0), n - 1))
        hi = int(min(max(np.floor(max(v) - 0.5) + reach + 1, 0), n - 1)) + 1
        if even:
            lo, hi = lo & ~1, (hi + 1) & ~1
        ends.append((lo, hi))
    (xa, xb), (ya, yb) = ends
    return xa, ya, xb - xa, yb - ya


def homography(src, dst):
    """The 3 x 3 float64 matrix, m22 = 1, that sends the four points src to dst (None if singular)."""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y]), b.append(u)
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y]), b.append(v)
    try:
        h = np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))
    except np.linalg.LinAlgError:
        return None
    return np.append(h, 1.0)


def random_homography(rng, H, Wd, oh, ow, strength=None, scales=(1.0, 0.01, 37.0)):
    """The output's corners to a rotated, scaled quadrilateral in or around the frame, each corner moved
    by up to `strength` of the quadrilateral's side; the nine entries times a common factor (which the
    quotient cancels), as float32.  None if degenerate."""
    if strength is None:
        strength = rng.choice([0.0, 0.1, 0.3, 0.45])
    src = np.array([[0, 0], [ow, 0], [ow, oh], [0, oh]], float)
    c = np.array([rng.uniform(-0.2 * Wd, 1.2 * Wd), rng.uniform(-0.2 * H, 1.2 * H)])
    s, th = np.exp(rng.uniform(-1.5, 2.5)), rng.uniform(-np.pi, np.pi)
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    dst = (src - [ow / 2, oh / 2]) @ Rm.T * s + c + rng.uniform(-strength, strength, (4, 2)) * s * np.array([ow, oh])
    h = homography(src, dst)
    if h is None:
        return None
    m = (h * rng.choice(scales)).astype(F32)
    return m if np.isfinite(m).all() else None


def accepted_homographies(rng, n, H, Wd, oh, ow, **kw):
    """n random homographies the plan accepts for this frame and output size."""
    out = []
    while len(out) < n:
        m = random_homography(rng, H, Wd, oh, ow, **kw)
        if m is not None and refusal(m, oh, ow, H, Wd) is None:
            out.append(m)
    return out
