"""Layout converters: the reference's planar fp32 <-> the library's blocked pixel-major layout (csrc/common.h; entries in
csrc/layer_ops.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import DT_BF16, DT_F32
from ._base import _TORCH_DT, _f32c, _ptr, _require_gpu, _stream


def to_pixel_major(x: torch.Tensor, dtype: int, channels: Optional[int] = None) -> torch.Tensor:
    """(N,C,H,W) fp32 planar -> the library's blocked pixel-major layout
    (N, H, ceil(W/32), Cp/8, 32, 8) in its element type (csrc/common.h).  The true width rides along as
    ``.pm_w`` (the padding pixels of the last 32-pixel segment are never read)."""
    _require_gpu(x)
    n, c, h, w = x.shape
    cp = channels or ((c + 15) // 16) * 16
    out = torch.empty((n, h, (w + 31) // 32, cp // 8, 32, 8), dtype=_TORCH_DT[dtype], device=x.device)
    out.pm_w = w
    lib = _lib.load()
    _lib.check(lib.vsr_planar_to_pm(dtype, _ptr(_f32c(x)), _ptr(out), n, c, h, w, cp, _stream()), "planar_to_pm")
    return out


def _pm_dims(x: torch.Tensor):
    n, h, ws, cp8, _, _ = x.shape
    return n, h, x.pm_w, cp8 * 8


def _pm_like(x: torch.Tensor, dtype=None) -> torch.Tensor:
    out = torch.empty_like(x) if dtype is None else torch.empty(x.shape, dtype=dtype, device=x.device)
    out.pm_w = x.pm_w
    return out


def from_pixel_major(x: torch.Tensor, channels: Optional[int] = None) -> torch.Tensor:
    """blocked pixel-major -> (N,C,H,W) fp32 planar."""
    _require_gpu(x)
    n, h, w, cp = _pm_dims(x)
    c = channels or cp
    dtype = DT_BF16 if x.dtype == torch.bfloat16 else DT_F32
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.vsr_pm_to_planar(dtype, _ptr(x), _ptr(out), n, c, h, w, cp, _stream()), "pm_to_planar")
    return out
