"""Reference of the mix stage (ccmi_mix; steps 4, 4e and 4m of the contract in include/ccmi.h) in torch CPU
float32 operations, one per product and sum, and, for the noise of step 4e, tests/noise_ref.py: the
counter-based generator at step 0, frame 0 (noise_ref.draw_uniforms(seed, 0, 0, index)) and its float64
Box-Muller transform.  A helper: no tests in it.  tests/test_decode_mix_ref.py pins it to independent
idioms on the CPU, tests/test_decode_mix_gpu.py compares the kernel with it.

A frame is a float32 tensor [3, oh, ow]: y_c(i, k) of the contract, the stored frame before step 4.
Rectangles are (x, y, w, h, value, sigma) with value one float or three, boxes (x, y, w, h), both in stored
coordinates.  Constant rectangles, the blend and the box are exact (the kernel must give these bits); a
noise rectangle's elements carry their float64 value and a bound instead (`Erased.want`, `Erased.tol`):
T + 2^-24 (|want| + T), T = noise_ref.gaussian_tol(u1, sigma) the derived bound of the draw and the second
term the rounding of the one float32 sum v_c + g."""
from collections import namedtuple

import numpy as np
import torch

import noise_ref

E24 = 2.0 ** -24

# e: float32 [3, oh, ow] after step 4e (a noise element holds its float64 value rounded to float32);
# noisy: bool, the elements whose final value is a draw; want / tol: float64, their value and bound
Erased = namedtuple("Erased", "e noisy want tol")


def three(v):
    v = [float(t) for t in v] if hasattr(v, "__len__") else [float(v)] * 3
    assert len(v) == 3
    return torch.tensor(v, dtype=torch.float32)


def normalise(y, scale, bias):
    """step 4: a_c = y_c scale[c] + bias[c], the product rounded before the sum"""
    assert y.dtype == torch.float32 and y.dim() == 3
    return y.mul(three(scale)[:, None, None]).add(three(bias)[:, None, None])


def inside(oh, ow, x, y, w, h):
    """bool [oh, ow]: x <= k < x + w and y <= i < y + h"""
    i, k = torch.arange(oh)[:, None], torch.arange(ow)[None, :]
    return (k >= x) & (k < x + w) & (i >= y) & (i < y + h)


def uniforms(seed, oh, ow):
    """(u1, u2), float64 [3, oh, ow]: the draws at index = (c oh + i) ow + k of generator `seed`"""
    u1, u2 = noise_ref.draw_uniforms(seed, 0, 0, np.arange(3 * oh * ow, dtype=np.uint64))
    return u1.reshape(3, oh, ow), u2.reshape(3, oh, ow)


def erase(a, rects, seed=0):
    """step 4e on a = normalise(y, ...): the rectangles in order, a later one winning -> Erased"""
    assert a.dtype == torch.float32 and a.dim() == 3
    _, oh, ow = a.shape
    e = a.clone()
    noisy = torch.zeros(3, oh, ow, dtype=torch.bool)
    want = torch.zeros(3, oh, ow, dtype=torch.float64)
    tol = torch.zeros(3, oh, ow, dtype=torch.float64)
    u = None
    for r in rects or ():
        x, y, w, h, value = r[:5]
        sigma = float(np.float32(r[5])) if len(r) > 5 else 0.0
        if w <= 0 or h <= 0:
            continue
        m = inside(oh, ow, x, y, w, h)[None].expand(3, oh, ow)
        v = three(value)[:, None, None].expand(3, oh, ow)
        if sigma == 0.0:
            e = torch.where(m, v, e)
            noisy = noisy & ~m
            continue
        if u is None:
            u = uniforms(seed, oh, ow)
        g = torch.from_numpy(noise_ref.gaussian(u[0], u[1], sigma))
        w64 = v.double() + g
        T = torch.from_numpy(np.broadcast_to(noise_ref.gaussian_tol(u[0], sigma), (3, oh, ow)).copy())
        e = torch.where(m, w64.float(), e)
        want = torch.where(m, w64, want)
        tol = torch.where(m, T + E24 * (w64.abs() + T), tol)
        noisy = noisy | m
    return Erased(e, noisy, want, tol)


def blend(a, b, lam):
    """step 4m, MixUp: (lam a) + (oml b), oml = 1.0f - lam in float32"""
    lam = np.float32(lam)
    oml = np.float32(1.0) - lam
    return a.mul(float(lam)).add(b.mul(float(oml)))


def cut(a, b, box):
    """step 4m, CutMix: b inside the box, a outside"""
    _, oh, ow = a.shape
    return torch.where(inside(oh, ow, *box)[None], b, a)


def batch(ys, scale, bias, erases=None, seeds=None, mixes=None):
    """Steps 4, 4e and 4m of a call: ys the frames' y (float32 [3, oh, ow] each), erases / seeds / mixes as
    erase= / erase_seed= / mix= of the *_model calls (per frame; None: none) -> (m, erased): m[j] the float32
    frame before step 5, erased[j] frame j's Erased (what a partner of j is blended with).  An element of
    m[j] is exact unless erased[j].noisy (or, under a blend or in a box, erased[partner].noisy) says so."""
    n = len(ys)
    erases = erases or [None] * n
    seeds = [seeds] * n if isinstance(seeds, int) else (seeds or [0] * n)
    mixes = mixes or [None] * n
    erased = [erase(normalise(ys[j], scale, bias), erases[j], seeds[j]) for j in range(n)]
    out = []
    for j in range(n):
        a = erased[j].e
        if mixes[j] is not None:
            p, what = mixes[j]
            b = erased[p].e
            assert b.shape == a.shape
            a = cut(a, b, what) if hasattr(what, "__len__") else blend(a, b, what)
        out.append(a)
    return out, erased
