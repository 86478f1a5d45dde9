"""JPEG round trip (csrc/jpeg_degrade.hip, libvsrlab_jpeg.so)."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib
from ._base import _STORAGE_DT, _ptr, _require_gpu, _stream


def jpeg_compress(x: torch.Tensor, quality: int) -> torch.Tensor:
    """``x`` after JPEG compression at ``quality`` (clamped to 1..100; 4:2:0 chroma) and decompression: what the reference's
    ``to_pil_image`` -> libjpeg -> ``to_tensor`` gives per frame, as the fixed-point specification of DESIGN section 11g, which
    equals PIL (libjpeg-turbo) bit for bit.  ``x``: (3, H, W) or (N, 3, H, W) RGB, fp32 or bf16, on the GPU, any
    strides; it is clamped to [0, 1] and not modified.  Returns a new contiguous tensor of the same shape and dtype whose values
    are k / 255, with no autograd history (the reference detaches its input).  Two kernel launches; there is no CPU fallback."""
    if x.dim() not in (3, 4) or x.shape[-3] != 3 or x.numel() == 0:
        raise ValueError(f"jpeg_compress: x must be (3, H, W) or (N, 3, H, W) and non-empty; got {tuple(x.shape)}")
    if x.dtype not in _STORAGE_DT:
        raise ValueError(f"jpeg_compress: x must be float32 or bfloat16; got {x.dtype}")
    _require_gpu(x)
    lib = _lib.load_jpeg()
    x4 = x.detach()
    x4 = x4[None] if x.dim() == 3 else x4
    n, _, h, w = (int(v) for v in x4.shape)
    y = torch.empty((n, 3, h, w), dtype=x.dtype, device=x.device)
    dt = _STORAGE_DT[x.dtype]
    L4 = ctypes.c_longlong * 4
    desc = _lib.JpegDesc(n, h, w, int(quality), dt, dt, L4(*x4.stride()), L4(*y.stride()))
    nbytes = int(lib.vsr_jpeg_workspace_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise RuntimeError(f"jpeg_compress: unsupported shape {tuple(x.shape)} (N <= 65535, H and W <= 32768)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.check(lib.vsr_jpeg_fwd(ctypes.byref(desc), _ptr(x4), _ptr(y), _ptr(ws), nbytes, _stream()), "jpeg_fwd")
    del ws
    return y[0] if x.dim() == 3 else y
