"""Distortion metrics on the GPU: MS-SSIM (value and gradient), its mix with the MSE, PSNR.

ccmi_msssim_f32 (include/ccmi.h states the metric: window, constants, pooling, combination) for
batches of frames; torch tensors are storage only.  A frame is `[3, H, W]` (4:4:4, or 4:2:0 with the
chroma taken at even rows and columns, as the training step's raw output) or a packed row of its
planes one after the other (Y, U, V as ccmi_post_f32 and the tensor decoder write them).

Rate-distortion results of streams tuned for MS-SSIM have not been measured.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Sequence

import torch

from . import check, lib, require_cuda

DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


class MsssimArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int), ("n_planes", C.c_int), ("n_scales", C.c_int), ("clamp", C.c_int),
        ("h", C.c_int * 3), ("w", C.c_int * 3), ("x", C.c_void_p), ("x_stride", C.c_int64),
        ("x_off", C.c_int64 * 3), ("x_pitch", C.c_int64 * 3), ("x_sub", C.c_int * 3),
        ("y", C.c_void_p), ("y_stride", C.c_int64), ("weights", C.c_float * 5), ("channel_weights", C.c_float * 3),
        ("alpha_mse", C.c_float), ("beta_ms", C.c_float), ("out", C.c_void_p), ("grad", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class TrainDist(C.Structure):
    _fields_ = [("n_scales", C.c_int), ("weights", C.c_float * 5), ("channel_weights", C.c_float * 3),
                ("alpha_mse", C.c_float), ("beta_ms", C.c_float), ("dist_out", C.c_void_p)]


def _bind():
    L = lib()
    if not getattr(L, "_ccmi_msssim_bound", False):
        L.ccmi_msssim_workspace_bytes.argtypes = [C.POINTER(MsssimArgs)]
        L.ccmi_msssim_workspace_bytes.restype = C.c_size_t
        L.ccmi_msssim_f32.argtypes = [C.POINTER(MsssimArgs), C.c_void_p]
        L.ccmi_msssim_f32.restype = C.c_int
        L._ccmi_msssim_bound = True
    return L


@dataclass(frozen=True)
class Distortion:
    """D = alpha_mse MSE + beta_ms (1 - MS-SSIM).  weights: one per scale (default: the first
    n_scales of the usual five, divided by their sum); channel_weights: one per plane (default 1/3
    each for 4:4:4, (4, 1, 1) / 6 for 4:2:0, the planes' sample counts)."""
    alpha_mse: float = 1.0
    beta_ms: float = 0.0
    n_scales: int = 5
    weights: Sequence[float] | None = None
    channel_weights: Sequence[float] | None = None

    def scale_weights(self) -> tuple:
        if self.weights is not None:
            if len(self.weights) != self.n_scales:
                raise ValueError(f"weights: {self.n_scales} values expected")
            return tuple(float(v) for v in self.weights)
        w = DEFAULT_WEIGHTS[:self.n_scales]
        return tuple(v / sum(w) for v in w)

    def plane_weights(self, yuv420: bool) -> tuple:
        if self.channel_weights is not None:
            if len(self.channel_weights) != 3:
                raise ValueError("channel_weights: 3 values expected")
            return tuple(float(v) for v in self.channel_weights)
        return (4 / 6, 1 / 6, 1 / 6) if yuv420 else (1 / 3, 1 / 3, 1 / 3)

    def train_struct(self, yuv420: bool, dist_out: torch.Tensor | None = None) -> TrainDist:
        """ccmi_train_dist of this distortion (ccmi_train_step_dist)."""
        d = TrainDist()
        d.n_scales = self.n_scales
        for i, v in enumerate(self.scale_weights()):
            d.weights[i] = v
        for i, v in enumerate(self.plane_weights(yuv420)):
            d.channel_weights[i] = v
        d.alpha_mse, d.beta_ms = float(self.alpha_mse), float(self.beta_ms)
        d.dist_out = None if dist_out is None else dist_out.data_ptr()
        return d


def plane_sizes(H: int, W: int, yuv420: bool) -> list:
    return [(H, W), (H // 2, W // 2), (H // 2, W // 2)] if yuv420 else [(H, W)] * 3


def distortion(x: torch.Tensor, y: torch.Tensor, dist: Distortion, yuv420: bool = False, grad=False,
               clamp: bool = True, size: tuple | None = None):
    """[B, 4] = (D, MS, MSE, min v_s) of frames x against y, and with grad also dD/dx (x's shape;
    unsampled chroma positions of a 4:2:0 `[B, 3, H, W]` input read 0; grad may be the buffer to
    write, of which only the sampled positions are touched).

    x: float32 `[B, 3, H, W]`, or packed rows `[B, n]` with size = (H, W); y: packed rows `[B, n]` or
    `[B, 3, H, W]` (4:4:4), or one shared row `[n]` / `[1, n]`."""
    require_cuda(x, y)
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("metrics: float32 tensors expected")
    x = x.contiguous()
    B = x.shape[0]
    a = MsssimArgs()
    if x.dim() == 4:
        if x.shape[1] != 3:
            raise ValueError("metrics: x is [B, 3, H, W] or packed [B, n]")
        H, W = int(x.shape[2]), int(x.shape[3])
        sizes = plane_sizes(H, W, yuv420)
        for p in range(3):
            a.x_off[p], a.x_pitch[p], a.x_sub[p] = p * H * W, W, 2 if (yuv420 and p) else 1
    elif x.dim() == 2 and size is not None:
        H, W = size
        sizes = plane_sizes(H, W, yuv420)
        o = 0
        for p, (h, w) in enumerate(sizes):
            a.x_off[p], a.x_pitch[p], a.x_sub[p] = o, w, 1
            o += h * w
        if x.shape[1] < o:
            raise ValueError(f"metrics: packed rows of {o} samples expected")
    else:
        raise ValueError("metrics: x is [B, 3, H, W], or packed [B, n] with size=(H, W)")
    n = sum(h * w for h, w in sizes)
    y = y.contiguous()
    shared = y.dim() == 1 or y.shape[0] == 1
    if y.numel() != n * (1 if shared else B):
        raise ValueError(f"metrics: y holds {y.numel()} samples, {n} per frame expected")
    a.batch, a.n_planes, a.n_scales, a.clamp = B, 3, dist.n_scales, int(bool(clamp))
    for p, (h, w) in enumerate(sizes):
        a.h[p], a.w[p] = h, w
    a.x, a.x_stride = x.data_ptr(), x.stride(0)
    a.y, a.y_stride = y.data_ptr(), 0 if shared else n
    for i, v in enumerate(dist.scale_weights()):
        a.weights[i] = v
    for i, v in enumerate(dist.plane_weights(yuv420)):
        a.channel_weights[i] = v
    a.alpha_mse, a.beta_ms = float(dist.alpha_mse), float(dist.beta_ms)
    out = torch.empty(B, 4, device=x.device)
    if isinstance(grad, torch.Tensor):  # the caller's buffer: only the sampled positions are written
        if grad.shape != x.shape or grad.dtype != torch.float32 or not grad.is_contiguous() or grad.device != x.device:
            raise ValueError("metrics: grad buffer must match x")
        g = grad
    else:
        g = torch.zeros_like(x) if grad else None
    a.out = out.data_ptr()
    a.grad = None if g is None else g.data_ptr()
    L = _bind()
    nws = L.ccmi_msssim_workspace_bytes(C.byref(a))
    ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nws
    check(L.ccmi_msssim_f32(C.byref(a), torch.cuda.current_stream(x.device).cuda_stream))
    return out if g is None else (out, g)


def ms_ssim(x: torch.Tensor, y: torch.Tensor, n_scales: int = 5, weights=None, channel_weights=None,
            yuv420: bool = False, grad: bool = False, clamp: bool = True, size: tuple | None = None):
    """MS-SSIM [B] of frames x against y (shapes as distortion()); with grad also d MS / dx."""
    d = Distortion(alpha_mse=0.0, beta_ms=1.0, n_scales=n_scales, weights=weights, channel_weights=channel_weights)
    r = distortion(x, y, d, yuv420=yuv420, grad=grad, clamp=clamp, size=size)
    return (r[0][:, 1], -r[1]) if grad else r[:, 1]


def psnr(mse, peak: float = 1.0):
    """10 log10(peak^2 / mse), of a float or a tensor."""
    if isinstance(mse, torch.Tensor):
        return 10 * torch.log10(peak * peak / mse.clamp_min(1e-20))
    return 10 * math.log10(peak * peak / max(float(mse), 1e-20))


__all__ = ["Distortion", "distortion", "ms_ssim", "psnr", "MsssimArgs", "TrainDist", "DEFAULT_WEIGHTS", "plane_sizes"]
