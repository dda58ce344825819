"""Torch restatement of the MS-SSIM distortion of include/ccmi.h (ccmi_msssim_args), generic in
dtype, the gradient by autograd; the float64 run is the reference of tests/test_msssim_gpu.py and
tests/test_train_msssim_gpu.py, the float32 run gives each case its own rounding scale e32.  No
package implements it here: tests/test_msssim_ref.py pins this file by closed forms.

The contract, restated:
  planes   X_p, Y_p of h[p] x w[p] samples, p < 3; sample (i, j) of X_p is
           x[off[p] + i sub[p] pitch[p] + j sub[p]]; clamp: X = min(max(x, 0), 1); Y as given
  window   g_k = exp(-(k - 5)^2 / 4.5) / sum, k = 0 .. 10, in double, rounded once to float32;
           separable, valid (no padding)
  scale s  mu = G*X ..., s_xx = G*(XX) - mu_x^2, s_xy = G*(XY) - mu_x mu_y,
           cs = (2 s_xy + C2) / (s_xx + s_yy + C2), l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1),
           C1 = 1e-4, C2 = 9e-4; v_s = mean cs (s < S - 1), mean cs l (s = S - 1)
  pooling  avg_pool2d(2, padding = size mod 2, count_include_pad = True) of X and Y
  result   MS_p = prod_s max(v_s, 0)^w_s (0, with gradient 0, when any v_s <= 0), MS = sum_p cw_p MS_p,
           MSE = sum of (X - Y)^2 over all samples of all planes / their number,
           D = alpha MSE + beta (1 - MS);  out = (D, MS, MSE, min v_s)
  workspace  al(n) = 4 n rounded up to 256; 2 al(B pyr) + al(2 B tiles) + al(16 B) [+ al(B pyr) +
           al(3 B pos) with a gradient], tiles of 22 x 32 positions
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 1e-4, 9e-4
DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TILE_H, TILE_W = 22, 32


def taps(dtype=torch.float64):
    t = [math.exp(-((k - 5) ** 2) / 4.5) for k in range(11)]
    s = sum(t)
    return torch.tensor(np.asarray([v / s for v in t], dtype=np.float64).astype(np.float32)).to(dtype)


def window(x, g):
    """valid separable window of [B, h, w]"""
    x = x[:, None]
    x = F.conv2d(x, g.view(1, 1, 1, 11))
    x = F.conv2d(x, g.view(1, 1, 11, 1))
    return x[:, 0]


def pool(x):
    """[B, h, w] -> [B, ceil(h / 2), ceil(w / 2)]"""
    h, w = x.shape[-2:]
    return F.avg_pool2d(x[:, None], 2, stride=2, padding=(h % 2, w % 2), count_include_pad=True)[:, 0]


def scale_terms(X, Y, g):
    mx, my = window(X, g), window(Y, g)
    sxx = window(X * X, g) - mx * mx
    syy = window(Y * Y, g) - my * my
    sxy = window(X * Y, g) - mx * my
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    l = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    return cs, l


def plane_v(X, Y, S, g):
    """[B, S] of v_s"""
    v = []
    for s in range(S):
        cs, l = scale_terms(X, Y, g)
        v.append((cs if s < S - 1 else cs * l).mean(dim=(1, 2)))
        if s < S - 1:
            X, Y = pool(X), pool(Y)
    return torch.stack(v, dim=1)


def default_weights(S):
    w = DEFAULT_WEIGHTS[:S]
    return tuple(v / sum(w) for v in w)


def evaluate(Xs, Ys, S, weights, cw, alpha, beta, clamp=True):
    """Xs, Ys: lists of [B, h_p, w_p] -> out [B, 4] (D, MS, MSE, min v_s), v [B, P, S]"""
    dt = Xs[0].dtype
    g = taps(dt).to(Xs[0].device)
    ms, se, n, vs = 0, 0, 0, []
    wt = torch.tensor(weights, dtype=torch.float64).to(dt).to(Xs[0].device)
    for p, (X, Y) in enumerate(zip(Xs, Ys)):
        if clamp:
            X = X.clamp(0, 1)
        v = plane_v(X, Y, S, g)
        vs.append(v)
        alive = (v > 0).all(dim=1)
        msp = torch.where(alive, (v.clamp_min(1e-30) ** wt).prod(dim=1), torch.zeros_like(v[:, 0]))
        ms = ms + float(np.float32(cw[p])) * msp
        se = se + ((X - Y) ** 2).sum(dim=(1, 2))
        n += X.shape[1] * X.shape[2]
    mse = se / n
    v = torch.stack(vs, dim=1)
    D = alpha * mse + beta * (1 - ms)
    return torch.stack([D, ms, mse, v.reshape(v.shape[0], -1).min(dim=1).values], dim=1), v


def size_chain(h, w, S):
    out = []
    for _ in range(S):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def workspace_bytes(B, sizes, S, grad):
    al = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731
    pyr = pos = tiles = 0
    for h, w in sizes:
        for s, (hs, ws) in enumerate(size_chain(h, w, S)):
            pyr += hs * ws if s else 0
            pos += (hs - 10) * (ws - 10)
            tiles += -(-(hs - 10) // TILE_H) * -(-(ws - 10) // TILE_W)
    n = 2 * al(B * pyr) + al(2 * B * tiles) + al(16 * B)
    if grad:
        n += al(B * pyr) + al(3 * B * pos)
    return n


# ---------------------------------------------------------------- the cases of the GPU tests
@dataclass(frozen=True)
class Case:
    name: str
    H: int
    W: int
    S: int
    layout: str = "packed444"      # packed444 | raw420 | packed420
    B: int = 1
    shared_y: bool = False
    clamp: bool = True
    alpha: float = 0.3
    beta: float = 0.7
    cw: tuple = None
    seed: int = 0

    @property
    def yuv420(self):
        return self.layout != "packed444"

    @property
    def sizes(self):
        c = (self.H // 2, self.W // 2) if self.yuv420 else (self.H, self.W)
        return [(self.H, self.W), c, c]

    @property
    def planes(self):
        """(off, pitch, sub) of each plane in a frame's row of x"""
        H, W = self.H, self.W
        if self.layout == "raw420":
            return [(0, W, 1), (H * W, W, 2), (2 * H * W, W, 2)]
        out, o = [], 0
        for h, w in self.sizes:
            out.append((o, w, 1))
            o += h * w
        return out

    @property
    def stride(self):
        return 3 * self.H * self.W if self.layout != "packed420" else sum(h * w for h, w in self.sizes)

    @property
    def channel_weights(self):
        return self.cw or ((4 / 6, 1 / 6, 1 / 6) if self.yuv420 else (1 / 3, 1 / 3, 1 / 3))

    @property
    def weights(self):
        return default_weights(self.S)


CASES = [
    Case("11x11s1", 11, 11, 1, seed=1),                          # one output position
    Case("12x27s1", 12, 27, 1),
    Case("21x23s2", 21, 23, 2),                                  # padding on both axes
    Case("22x45s2", 22, 45, 2),
    Case("41x43s3", 41, 43, 3),
    Case("161x161s5", 161, 161, 5),                              # the smallest legal five-scale frame
    Case("176x209s5", 176, 209, 5),
    Case("300x450s5", 300, 450, 5),                              # many workgroups per scale
    Case("55x75s2-tiles", 55, 75, 2),                            # 45 x 65 positions: 22 + 22 + 1 by 32 + 32 + 1
    Case("raw420-45x47s2", 45, 47, 2, layout="raw420", B=2),     # odd on both sides, chroma 22 x 23
    Case("packed420-44x46s2", 44, 46, 2, layout="packed420", B=2),
    Case("sharedy-21x23s2-b5", 21, 23, 2, B=5, shared_y=True),
    Case("noclamp-22x45s2", 22, 45, 2, clamp=False),
    Case("msonly-41x43s3", 41, 43, 3, alpha=0.0, beta=1.0),
    Case("mseonly-41x43s3", 41, 43, 3, alpha=1.0, beta=0.0),
    Case("cw-22x45s2", 22, 45, 2, cw=(0.5, 0.2, 0.3)),
    # the frames of tests/test_train_msssim_gpu.py (there the raw output is the network's)
    Case("train444-176x208s5", 176, 208, 5, layout="packed444", B=2, alpha=0.0, beta=1.0),
    Case("train420-176x208s4", 176, 208, 4, layout="raw420", B=2, alpha=0.0, beta=1.0),
]


def _plane(h, w, g):
    """a smooth target with texture, in [0.03, 0.97]"""
    i = torch.arange(h, dtype=torch.float64)[:, None]
    j = torch.arange(w, dtype=torch.float64)[None, :]
    f = torch.rand(4, generator=g, dtype=torch.float64) * 0.25 + 0.05
    ph = torch.rand(2, generator=g, dtype=torch.float64) * 6.28
    t = 0.5 + 0.3 * torch.sin(f[0] * i + ph[0]) * torch.cos(f[1] * j + ph[1]) + 0.1 * torch.sin(f[2] * (i + j)) \
        + 0.06 * torch.randn(h, w, generator=g, dtype=torch.float64)
    return t.clamp(0.03, 0.97)


@functools.lru_cache(maxsize=None)
def case_data(case: Case):
    """(x [B, stride] float32, y [B or 1, n] float32) on the CPU: raw = target + 0.03 N(0, 1), no raw
    value within 1e-4 of 0 or 1 (nudged), some outside [0, 1]; unsampled positions of x hold junk"""
    g = torch.Generator().manual_seed(1000 + case.seed + 7 * len(case.name) + case.H * case.W)
    By = 1 if case.shared_y else case.B
    n = sum(h * w for h, w in case.sizes)
    y = torch.empty(By, n, dtype=torch.float64)
    x = torch.rand(case.B, case.stride, generator=g, dtype=torch.float64) * 3 - 1  # junk
    for b in range(case.B):
        o = 0
        for (h, w), (off, pitch, sub) in zip(case.sizes, case.planes):
            if b < By:
                y[b, o:o + h * w] = _plane(h, w, g).reshape(-1)
            t = y[min(b, By - 1), o:o + h * w].view(h, w)
            raw = t + 0.03 * torch.randn(h, w, generator=g, dtype=torch.float64)
            x[b, plane_index(h, w, off, pitch, sub)] = raw.reshape(-1)
            o += h * w
    x = x.float()
    for edge in (0.0, 1.0):
        near = (x - edge).abs() < 1e-4
        x = torch.where(near, torch.full_like(x, edge) + torch.where(x >= edge, 2e-4, -2e-4), x)
    return x.contiguous(), y.float().contiguous()


def plane_index(h, w, off, pitch, sub):
    i = torch.arange(h)[:, None]
    j = torch.arange(w)[None, :]
    return (off + i * sub * pitch + j * sub).reshape(-1)


def run(case: Case, x, y, dtype):
    """out [B, 4], grad [B, stride] (0 off the sampled positions), v [B, 3, S] of the restatement
    in `dtype` on x, y (float32 tensors as the device gets them, any device)"""
    xd = x.detach().to(dtype).requires_grad_(True)
    yd = y.detach().to(dtype)
    Xs, Ys, o = [], [], 0
    for (h, w), (off, pitch, sub) in zip(case.sizes, case.planes):
        idx = plane_index(h, w, off, pitch, sub).to(x.device)
        Xs.append(xd[:, idx].view(-1, h, w))
        Ys.append(yd[:, o:o + h * w].view(-1, h, w).expand(x.shape[0], h, w))
        o += h * w
    out, v = evaluate(Xs, Ys, case.S, case.weights, case.channel_weights, case.alpha, case.beta, case.clamp)
    grad, = torch.autograd.grad(out[:, 0].sum(), xd)
    return out.detach(), grad, v.detach()


@dataclass
class Ref:
    out64: torch.Tensor
    g64: torch.Tensor
    v64: torch.Tensor
    e32: float          # largest |g32 - g64| over the largest |g64|
    eout: float         # largest |out32 - out64|
    sampled: torch.Tensor = field(repr=False, default=None)  # bool [stride]


def reference(case: Case, x, y) -> Ref:
    o64, g64, v64 = run(case, x, y, torch.float64)
    o32, g32, _ = run(case, x, y, torch.float32)
    e32 = float((g32.double() - g64).abs().max() / g64.abs().max())
    eout = float((o32.double() - o64).abs().max())
    m = torch.zeros(case.stride, dtype=torch.bool)
    for (h, w), (off, pitch, sub) in zip(case.sizes, case.planes):
        m[plane_index(h, w, off, pitch, sub)] = True
    return Ref(o64, g64, v64, e32, eout, m)


@functools.lru_cache(maxsize=None)
def case_ref(case: Case) -> Ref:
    return reference(case, *case_data(case))


E32_MAX = 2.0 ** -14


@functools.lru_cache(maxsize=None)
def out_bound():
    """16 x the largest float32-restatement distance of the four outputs over the standalone cases,
    floored at 2^-23"""
    return max(16 * max(case_ref(c).eout for c in CASES), 2.0 ** -23)
