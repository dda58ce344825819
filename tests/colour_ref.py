"""Step 3z of the ccmi_tensor_fmt contract (ccmi_colour, include/ccmi.h) restated with torch CPU
operations: every product, sum and difference is its own float32 torch operation in the order the
contract writes it, the frame's mean grey goes through int64 and float64.  The GPU tests put the
library's own float32 render of the same frames WITHOUT ops through this and compare bit for bit;
tests/test_decode_colour_ref.py pins it against plain float64 formulas."""
import numpy as np
import torch

BRIGHTNESS, SATURATION, CONTRAST, MATRIX = 0, 1, 2, 3  # CCMI_COL_*
NAMES = {"brightness": BRIGHTNESS, "saturation": SATURATION, "contrast": CONTRAST, "matrix": MATRIX}
GREY = (0.2989, 0.587, 0.114)


def _f(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32)


def _clamp(t):
    return t.clamp(0.0, 1.0)


def grey(x):
    """g = ((0.2989f x_0) + (0.587f x_1)) + (0.114f x_2)"""
    return (_f(GREY[0]) * x[0] + _f(GREY[1]) * x[1]) + _f(GREY[2]) * x[2]


def grey_sum(x):
    """S_j of the pixels x [3, h, w]: an int"""
    return int(torch.round(_clamp(grey(x)) * _f(65535.0)).to(torch.int64).sum())


def mean_grey(x):
    """m_j = (float)((double)S_j / ((double)N 65535.0))"""
    n = x.shape[-2] * x.shape[-1]
    return torch.tensor(grey_sum(x), dtype=torch.float64).div(float(n) * 65535.0).to(torch.float32)


def apply(x, ops):
    """x: [3, h, w] float32 (CPU), the frame after the geometry; ops: [(op, value)] as colour_ops=
    takes them.  Returns the frame after step 3z, float32."""
    x = x.detach().cpu().contiguous()
    assert x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 3
    x = [x[0], x[1], x[2]]
    for op, value in ops:
        op = NAMES.get(op, op)
        if op == MATRIX:
            m = np.asarray(value, dtype=np.float32).reshape(3, 4)
            x = [_clamp((((_f(m[c, 0]) * x[0]) + (_f(m[c, 1]) * x[1])) + (_f(m[c, 2]) * x[2])) + _f(m[c, 3])) for c in range(3)]
            continue
        f = np.float32(value)
        if op == BRIGHTNESS:
            x = [_clamp(_f(f) * x[c]) for c in range(3)]
            continue
        rest = np.float32(1.0) - f  # 1 - f, once, in float32
        if op == SATURATION:
            b = _f(rest) * grey(x)
        else:
            assert op == CONTRAST, op
            b = _f(rest) * mean_grey(torch.stack(x))
        x = [_clamp((_f(f) * x[c]) + b) for c in range(3)]
    out = torch.stack(x)
    assert out.dtype == torch.float32
    return out


def apply_f64(x, ops):
    """The same in plain float64 formulas (the mean a float64 mean of the clamped grey): what the
    restatement is checked against."""
    x = x.detach().cpu().to(torch.float64)
    w = torch.tensor(GREY, dtype=torch.float64)[:, None, None]
    for op, value in ops:
        op = NAMES.get(op, op)
        if op == MATRIX:
            m = torch.from_numpy(np.asarray(value, dtype=np.float64).reshape(3, 4))
            x = (torch.einsum("ck,khw->chw", m[:, :3], x) + m[:, 3, None, None]).clamp(0, 1)
        elif op == BRIGHTNESS:
            x = (float(value) * x).clamp(0, 1)
        elif op == SATURATION:
            x = (float(value) * x + (1 - float(value)) * (w * x).sum(0)).clamp(0, 1)
        else:
            x = (float(value) * x + (1 - float(value)) * (w * x).sum(0).clamp(0, 1).mean()).clamp(0, 1)
    return x
