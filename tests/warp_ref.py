"""The warping steps 3a-3d of the ccmi_warp contract (include/ccmi.h) in numpy float32, one rounded
operation at a time, and the plan's window rule: the reference of tests/test_decode_warp_gpu.py
and tests/test_decode_warp_abi.py, pinned by tests/test_decode_warp_ref.py against torch's
grid_sample in float64.  Nothing here calls the library."""
import numpy as np

F32 = np.float32
PAD_FILL, PAD_EDGE = 0, 1


def positions(m, oh, ow, dtype=F32):
    """Steps 3a-3b for every output pixel: (x0, fx, y0, fy), each [oh, ow]; x0 / y0 int64.  m: the
    six matrix entries.  dtype float32 is the contract, float64 the definition it rounds."""
    m = np.asarray(m, F32).reshape(6).astype(dtype)
    half = dtype(0.5)
    cx = (np.arange(ow).astype(dtype) + half)[None, :]
    cy = (np.arange(oh).astype(dtype) + half)[:, None]
    xs = ((m[0] * cx) + (m[1] * cy)) + m[2]
    ys = ((m[3] * cx) + (m[4] * cy)) + m[5]
    assert xs.dtype == dtype and ys.dtype == dtype and xs.shape == (oh, ow)
    u, v = xs - half, ys - half
    x0f, y0f = np.floor(u), np.floor(v)
    fx, fy = u - x0f, v - y0f
    assert fx.dtype == dtype
    return x0f.astype(np.int64), fx, y0f.astype(np.int64), fy


def taps_in_frame(m, oh, ow, H, W):
    """(ys, xs) of every tap of the float32 contract that lies in the frame (the pixels a window must hold)."""
    x0, _, y0, _ = positions(m, oh, ow)
    ys = np.concatenate([(y0 + a).ravel() for a in (0, 1) for _ in (0, 1)])
    xs = np.concatenate([(x0 + b).ravel() for _ in (0, 1) for b in (0, 1)])
    ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    return ys[ok], xs[ok]


def warp(q, m, oh, ow, pad=PAD_FILL, fill=(0.0, 0.0, 0.0), dtype=F32):
    """q: [3, H, W] (steps 1-3 over the whole frame) -> r' [3, oh, ow]: steps 3a-3d, every product,
    sum and difference one operation of `dtype` in the contract's order."""
    q = np.ascontiguousarray(q).astype(dtype)
    assert q.ndim == 3
    C, H, W = q.shape
    x0, fx, y0, fy = positions(m, oh, ow, dtype)
    fillv = np.asarray(fill, F32).reshape(-1).astype(dtype)
    if fillv.size == 1:
        fillv = np.repeat(fillv, C)
    one = dtype(1)

    def tap(a, b):
        yy, xx = y0 + a, x0 + b
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        t = q[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]  # [C, oh, ow]; EDGE: this
        if pad == PAD_FILL:
            t = np.where(inside[None], t, fillv[:, None, None])
        else:
            assert pad == PAD_EDGE
        return t.astype(dtype)
    gx, gy = one - fx, one - fy
    top = (tap(0, 0) * gx) + (tap(0, 1) * fx)
    bot = (tap(1, 0) * gx) + (tap(1, 1) * fx)
    r = (top * gy) + (bot * fy)
    assert r.dtype == dtype
    return r


def window(m, oh, ow, H, W, even=False):
    """The plan's window (x, y, w, h) of an H x W frame, in float64 from the float32 matrix: the
    positions at the four corner pixel centres, columns floor(min xs - 0.5) - 1 ..
    floor(max xs - 0.5) + 2 and rows alike, each end clamped into the frame; even: grown to even
    x, y, w, h (420 samples; H and W even)."""
    m = np.asarray(m, F32).reshape(6).astype(np.float64)
    ends = []
    for r, n in ((0, W), (1, H)):
        v = [m[3 * r] * cx + m[3 * r + 1] * cy + m[3 * r + 2] for cx in (0.5, ow - 0.5) for cy in (0.5, oh - 0.5)]
        lo = int(min(max(np.floor(min(v) - 0.5) - 1, 0), n - 1))
        hi = int(min(max(np.floor(max(v) - 0.5) + 2, 0), n - 1)) + 1
        if even:
            lo, hi = lo & ~1, (hi + 1) & ~1
        ends.append((lo, hi))
    (x0, x1), (y0, y1) = ends
    return x0, y0, x1 - x0, y1 - y0


def reach(m, oh, ow):
    """M of the float32 bound: the larger of |m00| out_w + |m01| out_h + |m02| and the second row's sum."""
    m = np.abs(np.asarray(m, F32).reshape(6).astype(np.float64))
    return max(m[0] * ow + m[1] * oh + m[2], m[3] * ow + m[4] * oh + m[5])
