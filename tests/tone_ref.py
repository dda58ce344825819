"""Step 3x of the ccmi_tensor_fmt contract (ccmi_tone, include/ccmi.h) restated in numpy: every product,
sum, difference and division is its own np.float32 operation in the order the contract writes it, the
statistics go through integers (and the contrast mean through float64, as in step 3z).  The GPU tests put
the library's own float32 render of the same frames WITHOUT tone ops and filter (same mirror: the frame
as stored) through colour_ref where there are colour ops, through this, then through filter_ref, and
compare bit for bit; tests/test_decode_tone_ref.py pins it against independent torch restatements."""
import numpy as np

BRIGHTNESS, SATURATION, CONTRAST, MATRIX, SOLARIZE, POSTERIZE, AUTOCONTRAST, EQUALIZE, SHARPNESS = range(9)  # CCMI_TONE_*
NAMES = {"brightness": BRIGHTNESS, "saturation": SATURATION, "contrast": CONTRAST, "matrix": MATRIX, "solarize": SOLARIZE,
         "posterize": POSTERIZE, "autocontrast": AUTOCONTRAST, "equalize": EQUALIZE, "sharpness": SHARPNESS}
MAX_OPS = 8
GREY = (np.float32(0.2989), np.float32(0.587), np.float32(0.114))
F0, F1 = np.float32(0.0), np.float32(1.0)
W_CENTRE, W_OTHER = np.float32(5.0 / 13.0), np.float32(1.0 / 13.0)


def clamp(t):
    """to [0, 1]; a NaN clamps to 0"""
    with np.errstate(invalid="ignore"):
        return np.where(t > F0, np.minimum(t, F1), F0).astype(np.float32)


def grey(x):
    return (GREY[0] * x[0] + GREY[1] * x[1]) + GREY[2] * x[2]


def mean_grey(x):
    """m_j of step 3z: the integer sum S_j, then (float)((double)S_j / ((double)N 65535.0))"""
    s = int(np.rint(clamp(grey(x)) * np.float32(65535.0)).astype(np.int64).sum())
    return np.float32(np.float64(s) / (np.float64(x.shape[-2] * x.shape[-1]) * 65535.0))


def quantise(x):
    """q = (int) rintf(clamp(x) 255.0f), ties to even"""
    return np.rint(clamp(x) * np.float32(255.0)).astype(np.int64)


def equalize_lut(hist):
    """The LUT of one channel from its 256-bin histogram, in Python integers"""
    hist = [int(v) for v in hist]
    n = sum(hist)
    last = max(t for t in range(256) if hist[t])
    step = (n - hist[last]) // 255
    if step == 0:
        return np.arange(256, dtype=np.int64)
    lut, run = [0], 0
    for t in range(1, 256):
        run += hist[t - 1]
        lut.append(min(255, (run + step // 2) // step))
    return np.array(lut, dtype=np.int64)


def solarize(x, th):
    return np.where(x >= np.float32(th), F1 - x, x).astype(np.float32)


def posterize(x, bits):
    L = np.float32(2 ** int(bits))
    return (np.minimum(np.maximum(np.floor(clamp(x) * L), F0), L - F1) * (F1 / L)).astype(np.float32)


def autocontrast(x):
    out = x.copy()
    for c in range(3):
        v = clamp(x[c])
        lo, hi = v.min(), v.max()
        if hi != lo:
            s = F1 / (hi - lo)
            out[c] = clamp((x[c] - lo) * s)
    return out


def equalize(x):
    out = np.empty_like(x)
    for c in range(3):
        q = quantise(x[c])
        lut = equalize_lut(np.bincount(q.ravel(), minlength=256))
        out[c] = lut[q].astype(np.float32) / np.float32(255.0)
    return out


def sharpness(x, f):
    f = np.float32(f)
    g = F1 - f
    _, h, w = x.shape
    if h <= 2 or w <= 2:
        return x.copy()
    b = x.copy()
    acc = np.zeros((3, h - 2, w - 2), dtype=np.float32)
    for di in (-1, 0, 1):
        for dk in (-1, 0, 1):
            wt = W_CENTRE if di == 0 and dk == 0 else W_OTHER
            acc = acc + wt * x[:, 1 + di: h - 1 + di, 1 + dk: w - 1 + dk]
    b[:, 1:-1, 1:-1] = acc
    return clamp((f * x) + (g * b))


def apply(x, ops):
    """x: [3, h, w] float32 (a CPU tensor or an array), the staged frame; ops: [(op, value)] as tone_ops=
    takes them.  Returns the frame after step 3x: a float32 torch tensor."""
    import torch
    x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x)
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[0] == 3 and len(ops) <= MAX_OPS
    x = x + F0
    for op, value in ops:
        op = NAMES.get(op, op)
        if op == MATRIX:
            m = np.asarray(value, dtype=np.float32).reshape(3, 4)
            x = np.stack([clamp((((m[c, 0] * x[0]) + (m[c, 1] * x[1])) + (m[c, 2] * x[2])) + m[c, 3]) for c in range(3)])
        elif op == BRIGHTNESS:
            x = clamp(np.float32(value) * x)
        elif op in (SATURATION, CONTRAST):
            f = np.float32(value)
            b = (F1 - f) * (grey(x) if op == SATURATION else mean_grey(x))
            x = clamp((f * x) + b)
        elif op == SOLARIZE:
            x = solarize(x, value)
        elif op == POSTERIZE:
            x = posterize(x, value)
        elif op == AUTOCONTRAST:
            x = autocontrast(x)
        elif op == EQUALIZE:
            x = equalize(x)
        else:
            assert op == SHARPNESS, op
            x = sharpness(x, value)
        assert x.dtype == np.float32, op
    return torch.from_numpy(np.ascontiguousarray(x))
