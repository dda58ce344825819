"""Steps 3y-0 .. 3y-2 of the ccmi_tensor_fmt contract (ccmi_filter, include/ccmi.h) restated with torch
CPU operations: every product and sum is its own float32 torch operation in the order the contract
writes it (the sums from 0.0f over d ascending).  The GPU tests put the library's own float32 render of
the same frames WITHOUT a filter (same mirror: the frame as stored) through this, after colour_ref where
there are ops, and compare bit for bit; tests/test_decode_filter_ref.py pins it against float64 sums,
F.pad's reflection and torch.where."""
import numpy as np
import torch

MAX_RADIUS = 15  # CCMI_FLT_MAX_RADIUS


def refl(a, n):
    """refl(a, n) of the contract, for an int or an int64 tensor a"""
    if n == 1:
        return a * 0
    p = 2 * (n - 1)
    m = a % p  # Python's and torch's remainder take the divisor's sign: m in [0, p)
    if isinstance(m, torch.Tensor):
        return torch.where(m < n, m, p - m)
    return m if m < n else p - m


def _f(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32)


def _pass(x, taps, dim):
    """sum_{d = -r .. r} w_|d| x(.., refl(k + d, n), ..) along dim, from 0.0f over d ascending"""
    r = len(taps) - 1
    n = x.shape[dim]
    at = torch.arange(n, dtype=torch.int64)
    t = torch.zeros_like(x)
    for d in range(-r, r + 1):
        t = t + _f(taps[abs(d)]) * x.index_select(dim, refl(at + d, n))
    return t


def blur(x, taps):
    """3y-1 for x [3, h, w] float32 and the half taps w_0 .. w_r (r >= 1)"""
    return _pass(_pass(x, taps, 2), taps, 1).clamp(0.0, 1.0)


def solarize(y, th):
    """3y-2: y >= th ? 1.0f - y : y"""
    return torch.where(y >= _f(th), _f(1.0) - y, y)


def apply(x, taps=None, th=None):
    """x: [3, h, w] float32 (CPU), the frame after step 3z as it will be stored; taps: None, or the
    half taps (a centre tap alone, like None, is radius 0: no blur); th: None or the threshold (above
    1: off).  Returns the frame after step 3y-2, float32."""
    x = x.detach().cpu().contiguous()
    assert x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 3
    y = x + _f(0.0)  # 3y-0
    taps = None if taps is None else np.asarray(taps, dtype=np.float32)
    if taps is not None and taps.size > 1:
        assert taps.ndim == 1 and taps.size - 1 <= MAX_RADIUS
        y = blur(y, taps)
    if th is not None and np.float32(th) <= np.float32(1.0):
        y = solarize(y, th)
    assert y.dtype == torch.float32
    return y


def takes_stage(taps, th):
    return (taps is not None and len(taps) > 1) or (th is not None and np.float32(th) <= np.float32(1.0))


def blur_f64(x, taps):
    """3y-1 in float64, the same sums (what the restatement is checked against)"""
    x = x.detach().cpu().to(torch.float64)
    w = [float(np.float32(v)) for v in taps]
    r = len(w) - 1
    for dim in (2, 1):
        n = x.shape[dim]
        at = torch.arange(n, dtype=torch.int64)
        t = torch.zeros_like(x)
        for d in range(-r, r + 1):
            t = t + w[abs(d)] * x.index_select(dim, refl(at + d, n))
        x = t
    return x.clamp(0.0, 1.0)
