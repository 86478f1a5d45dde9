"""What every op family shares: the compute-dtype rule, the GPU-only guard, stream and pointer marshalling for the C ABI, the
dtype maps, the widths of the HIP path and the backward-once guard of the ops that keep their gradient state in a workspace."""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import torch

from .._lib import DT_BF16, DT_F32


_DT = {"fp32": DT_F32, "float32": DT_F32, "f32": DT_F32, "bf16": DT_BF16, "bfloat16": DT_BF16}
_TORCH_DT = {DT_F32: torch.float32, DT_BF16: torch.bfloat16}
_STORAGE_DT = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}     # the element type of a tensor stored as it is


def resolve_dtype(compute_dtype: Optional[str] = None) -> int:
    """Internal activation dtype: explicit argument > $VSRLAB_AMD_DTYPE > bf16 under autocast > fp32.

    (The reference runs its forward under ``torch.cuda.amp.autocast()``, train.py:93; the
    MI355X build maps that to bf16 storage / fp32 accumulate.)"""
    name = compute_dtype or os.environ.get("VSRLAB_AMD_DTYPE")
    if name is None:
        name = "bf16" if torch.is_autocast_enabled("cuda") else "fp32"
    if name not in _DT:
        raise ValueError(f"unknown compute dtype {name!r}; use 'fp32' or 'bf16'")
    return _DT[name]


def _require_gpu(*tensors: torch.Tensor) -> None:
    for x in tensors:
        if not x.is_cuda:
            raise RuntimeError("vsrlab_amd runs on MI355X only: got a CPU tensor and there is no CPU fallback "
                               "(the CPU restatement lives in oracle/ and is test infrastructure)")


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(x: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if x is None else x.data_ptr())


def _ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, x in enumerate(tensors):
        arr[i] = 0 if x is None else x.data_ptr()
    return arr


def _f32c(x: torch.Tensor) -> torch.Tensor:
    return x.detach().to(torch.float32).contiguous()


MID_CHANNELS = (16, 32, 64)          # the widths of the HIP path: 64 on the whole-path entries, 16 / 32 on the narrow ones


def _check_width(c: int, what: str) -> None:
    if c not in MID_CHANNELS:
        raise NotImplementedError(f"the HIP {what} is built for mid_channels 16, 32 or 64, not {c}")


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _backward_once(ctx, op: str, has_gradient: bool = True, noun: Optional[str] = None) -> None:
    """What the backward of an op that keeps its gradient state in a workspace refuses: a double backward, a second backward,
    and a backward through a forward that kept nothing for one.  `noun`: the op in words, where the messages use them."""
    if torch.is_grad_enabled():
        raise RuntimeError(f"vsrlab_amd: {op} has no double backward (create_graph=True is not supported)")
    if ctx.backward_done:
        raise RuntimeError(f"vsrlab_amd: trying to backward through {f'the {noun}' if noun else op} a second time")
    if not has_gradient:
        raise RuntimeError(f"vsrlab_amd: backward through a {noun or op} that ran without a gradient")
