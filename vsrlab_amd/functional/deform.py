"""Deformable convolution and VRT's flow-guided alignment
(reference: core/modules/conv.py:33-80, vsr/models/VRT/modules/deform_conv.py:133-145; csrc/deform_conv.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import DT_F32
from ._base import _backward_once, _f32c, _ptr, _require_gpu, _stream, resolve_dtype


def _deform_desc(x_shape, cout: int, dg: int, modulated: bool, flow_guided: bool, mrm: float, dtype: int):
    from .._lib import DeformDesc
    n, cin, h, w = x_shape
    return DeformDesc(int(n), int(cin), int(cout), int(h), int(w), int(dg), int(modulated), int(flow_guided), float(mrm), int(dtype))


def deform_conv_workspace_bytes(x_shape, cout: int, deform_groups: int, dtype: int = DT_F32, need_backward: bool = False) -> int:
    """Device workspace of one ``vsr_deform_conv_fwd`` (or ``_bwd``) call; 0: unsupported shape.  Host arithmetic only."""
    desc = _deform_desc(x_shape, cout, deform_groups, True, False, 0.0, dtype)
    return int(_lib.load().vsr_deform_conv_workspace_bytes(ctypes.byref(desc), int(bool(need_backward))))


class _DeformConvFn(torch.autograd.Function):
    """y = deform_conv2d(x, offset, weight, bias, 1, 1, 1, mask); flow-guided: ``om`` is the raw conv_offset output and ``flow`` is
    given.  The backward recomputes the columns from the saved inputs; d x is summed with fp32 atomic adds (reproducible to
    rounding), every other gradient is bit-identical across runs."""

    @staticmethod
    def forward(ctx, x, om, mask, flow, weight, bias, meta):
        dtype, dg, mrm, need_bwd = meta
        lib = _lib.load()
        x32, om32, w32 = _f32c(x), _f32c(om), _f32c(weight)
        mask32 = None if mask is None else _f32c(mask)
        flow32 = None if flow is None else _f32c(flow)
        b32 = None if bias is None else _f32c(bias)
        n, cin, h, w = x32.shape
        cout = w32.shape[0]
        desc = _deform_desc(x32.shape, cout, dg, mask is not None or flow is not None, flow is not None, mrm, dtype)
        nbytes = int(lib.vsr_deform_conv_workspace_bytes(ctypes.byref(desc), 0))
        if nbytes == 0:
            raise RuntimeError("vsrlab_amd: deform_conv2d: unsupported shape (Cin, Cout <= 192, deformable groups padded to 8 / "
                               f"multiples of 16 channels within 192): x {tuple(x32.shape)}, Cout {cout}, deform_groups {dg}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x32.device)
        y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x32.device)
        _lib.check(lib.vsr_deform_conv_fwd(ctypes.byref(desc), _ptr(x32), _ptr(om32), _ptr(mask32), _ptr(flow32), _ptr(w32), _ptr(b32),
                                           _ptr(y), _ptr(ws), nbytes, _stream()), "deform_conv_fwd")
        del ws
        ctx.need_bwd = need_bwd
        if need_bwd:
            ctx.saved = (x32, om32, mask32, flow32, w32)
        ctx.desc = desc
        ctx.backward_done = False
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (x, om, mask, flow, weight, bias))
        return y

    @staticmethod
    def backward(ctx, gy):
        _backward_once(ctx, "deform_conv2d", ctx.need_bwd)
        lib = _lib.load()
        (x32, om32, mask32, flow32, w32), ctx.saved, ctx.backward_done = ctx.saved, None, True
        desc = ctx.desc
        dev = x32.device
        gy = _f32c(gy)
        need = ctx.needs_input_grad
        gx = torch.empty_like(x32) if need[0] else None
        gom = torch.empty_like(om32) if need[1] else None
        gmask = torch.empty_like(mask32) if (mask32 is not None and need[2]) else None
        gflow = torch.empty_like(flow32) if (flow32 is not None and need[3]) else None
        gw = torch.empty_like(w32) if need[4] else None
        gb = torch.empty(w32.shape[0], dtype=torch.float32, device=dev) if (ctx.dtypes[5] is not None and need[5]) else None
        nbytes = int(lib.vsr_deform_conv_workspace_bytes(ctypes.byref(desc), 1))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.vsr_deform_conv_bwd(ctypes.byref(desc), _ptr(x32), _ptr(om32), _ptr(mask32), _ptr(flow32), _ptr(w32), _ptr(gy),
                                           _ptr(gx), _ptr(gom), _ptr(gmask), _ptr(gflow), _ptr(gw), _ptr(gb), _ptr(ws), nbytes, _stream()),
                   "deform_conv_bwd")
        del ws
        outs = [g if g is None else g.to(dt) for g, dt in zip((gx, gom, gmask, gflow, gw, gb), ctx.dtypes)]
        return (*outs, None)


def _deform_checks(x, weight, bias, om_channels_per_group, om, what):
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{what}: x must be (N, Cin, H, W) and weight (Cout, Cin, 3, 3); got {tuple(x.shape)} and {tuple(weight.shape)}")
    n, cin, h, w = x.shape
    if tuple(weight.shape[1:]) != (cin, 3, 3):
        raise ValueError(f"{what}: weight must be (Cout, {cin}, 3, 3) (3x3 kernel, groups 1); got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"{what}: bias must be ({weight.shape[0]},); got {tuple(bias.shape)}")
    if om.dim() != 4 or om.shape[0] != n or tuple(om.shape[2:]) != (h, w) or om.shape[1] % om_channels_per_group or om.shape[1] == 0:
        raise ValueError(f"{what}: expected (N, {om_channels_per_group} * deform_groups, {h}, {w}); got {tuple(om.shape)}")
    dg = om.shape[1] // om_channels_per_group
    if cin % dg:
        raise ValueError(f"{what}: the {dg} deformable groups do not divide the {cin} input channels")
    return dg


def deform_conv2d(x: torch.Tensor, offset: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride=1, padding=1,
                  dilation=1, mask: Optional[torch.Tensor] = None, compute_dtype: Optional[str] = None) -> torch.Tensor:
    """``torchvision.ops.deform_conv2d`` on the HIP path for what the reference instantiates: 3x3, stride 1, padding 1,
    dilation 1, groups 1.  Offsets and masks stay fp32 whatever ``compute_dtype``.  Differentiable in x, offset, mask, weight, bias."""
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if pair(stride) != (1, 1) or pair(padding) != (1, 1) or pair(dilation) != (1, 1):
        raise NotImplementedError(f"HIP deform_conv2d: stride 1, padding 1, dilation 1 (got {stride}, {padding}, {dilation})")
    dg = _deform_checks(x, weight, bias, 18, offset, "deform_conv2d offset")
    if mask is not None and tuple(mask.shape) != (x.shape[0], 9 * dg, x.shape[2], x.shape[3]):
        raise ValueError(f"deform_conv2d: mask must be ({x.shape[0]}, {9 * dg}, {x.shape[2]}, {x.shape[3]}); got {tuple(mask.shape)}")
    tensors = [t for t in (x, offset, weight, bias, mask) if t is not None]
    _require_gpu(*tensors)
    need_bwd = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    return _DeformConvFn.apply(x, offset, mask, None, weight, bias, (resolve_dtype(compute_dtype), dg, 0.0, need_bwd))


def flow_guided_deform_conv(x: torch.Tensor, out: torch.Tensor, flow: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                            max_residue_magnitude: float, compute_dtype: Optional[str] = None) -> torch.Tensor:
    """``DCNv2PackFlowGuided.forward`` after its offset convolutions (deform_conv.py:135-145), fused: ``out`` is the raw output
    of ``conv_offset`` (N, 27 * deform_groups, H, W), ``flow`` (N, 2, H, W) with channel 0 = x.  The offsets
    ``mrm * tanh(out) + flow`` and the masks ``sigmoid(out)`` are formed inside the kernels and never stored."""
    dg = _deform_checks(x, weight, bias, 27, out, "flow_guided_deform_conv out")
    if tuple(flow.shape) != (x.shape[0], 2, x.shape[2], x.shape[3]):
        raise ValueError(f"flow_guided_deform_conv: flow must be ({x.shape[0]}, 2, {x.shape[2]}, {x.shape[3]}); got {tuple(flow.shape)}")
    tensors = [t for t in (x, out, flow, weight, bias) if t is not None]
    _require_gpu(*tensors)
    need_bwd = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    return _DeformConvFn.apply(x, out, None, flow, weight, bias,
                               (resolve_dtype(compute_dtype), dg, float(max_residue_magnitude), need_bwd))


def flow_guided_offset_mask(out: torch.Tensor, flow: torch.Tensor, max_residue_magnitude: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (offset, mask) pair ``flow_guided_deform_conv`` forms on the fly, as tensors and with the same bits (no autograd):
    for inspection and for checking the fused call against ``deform_conv2d``."""
    _require_gpu(out, flow)
    n, c, h, w = out.shape
    if c % 27:
        raise ValueError(f"flow_guided_offset_mask: out must have 27 * deform_groups channels; got {c}")
    dg = c // 27
    desc = _deform_desc((n, dg, h, w), 1, dg, True, True, float(max_residue_magnitude), DT_F32)
    out32, flow32 = _f32c(out), _f32c(flow)
    offset = torch.empty((n, 18 * dg, h, w), dtype=torch.float32, device=out.device)
    mask = torch.empty((n, 9 * dg, h, w), dtype=torch.float32, device=out.device)
    _lib.check(_lib.load().vsr_deform_offset_mask(ctypes.byref(desc), _ptr(out32), _ptr(flow32), _ptr(offset), _ptr(mask), _stream()),
               "deform_offset_mask")
    return offset, mask
