"""PSNR / SSIM in one pass (reference: piqa.PSNR / piqa.SSIM behind core/metrics.py, fed by core/utils.py:242-252;
csrc/metrics.hip)."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from .. import _lib
from ._base import _f32c, _ptr, _require_gpu, _stream


class PsnrSsimSums(NamedTuple):
    """Per-image results of ``psnr_ssim`` (fp64, shape (N,)): ``mse`` = mean of (x - y)^2 over (C, H, W), ``ssim`` = mean of the
    SSIM map over (C, H - ws + 1, W - ws + 1); ``sq_err_sum`` and ``ss_sum`` are the kernel's own sums that the two were divided from."""
    mse: torch.Tensor
    ssim: torch.Tensor
    sq_err_sum: torch.Tensor
    ss_sum: torch.Tensor


def psnr_ssim(x: torch.Tensor, y: torch.Tensor, *, window_size: int = 11, sigma: float = 1.5, value_range: float = 1.0,
              k1: float = 0.01, k2: float = 0.03, clamp: Optional[Tuple[float, float]] = None) -> PsnrSsimSums:
    """Mean squared error and SSIM (piqa's definition: Gaussian window, no padding, no unbiasing) of every image of a batch in one
    kernel pass over ``x`` (prediction) and ``y`` (target).  Both are (..., C, H, W); the leading dimensions are flattened to the
    batch.  ``clamp=(lo, hi)`` clamps ``x`` inside the kernel's load (``compute_metric``'s ``sr.clamp(0, 1)``); ``y`` is never clamped.

    The inputs are detached (nothing here is differentiated).  A tensor that is not fp32 is converted with ``.float()`` and one that
    is not contiguous is copied with ``.contiguous()``: an fp32 contiguous tensor is read where it lies.  There is no CPU fallback."""
    if x.shape != y.shape or x.dim() < 3:
        raise ValueError(f"psnr_ssim: x and y must have one shape (..., C, H, W); got {tuple(x.shape)} and {tuple(y.shape)}")
    _require_gpu(x, y)
    c, h, w = (int(v) for v in x.shape[-3:])
    ws = int(window_size)
    if ws % 2 == 0 or not 3 <= ws <= 15:
        raise ValueError(f"psnr_ssim: window_size must be odd and within 3..15, got {window_size}")
    if h < ws or w < ws:
        raise ValueError(f"psnr_ssim: images of {h} x {w} are smaller than the {ws} x {ws} SSIM window")
    if x.numel() == 0:
        raise ValueError(f"psnr_ssim: empty input of shape {tuple(x.shape)}")
    if not sigma > 0:
        raise ValueError(f"psnr_ssim: sigma must be positive, got {sigma}")
    if clamp is not None and not float(clamp[0]) <= float(clamp[1]):
        raise ValueError(f"psnr_ssim: clamp must be (lo, hi) with lo <= hi, got {clamp}")
    x4, y4 = _f32c(x).reshape(-1, c, h, w), _f32c(y).reshape(-1, c, h, w)
    n = x4.shape[0]
    lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    desc = _lib.MetricsDesc(n * c, c, h, w, ws, float(sigma), (float(k1) * float(value_range)) ** 2, (float(k2) * float(value_range)) ** 2,
                            int(clamp is not None), lo, hi)
    lib = _lib.load()
    nbytes = int(lib.vsr_metrics_scratch_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise ValueError(f"psnr_ssim: unsupported problem: {n} images of {c} x {h} x {w}, window {ws}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x4.device)
    sums = torch.empty((n, 2), dtype=torch.float64, device=x4.device)
    _lib.check(lib.vsr_psnr_ssim(ctypes.byref(desc), _ptr(x4), _ptr(y4), _ptr(sums), _ptr(scratch), nbytes, _stream()), "psnr_ssim")
    return PsnrSsimSums(mse=sums[:, 1] / float(c * h * w), ssim=sums[:, 0] / float(c * (h - ws + 1) * (w - ws + 1)),
                        sq_err_sum=sums[:, 1], ss_sum=sums[:, 0])
