"""flow_warp (reference: vsr/models/RealBasicVSR/modules/spynet.py:95-106; entries in csrc/layer_ops.hip), then the integer-tap warps and
VRT's aligned input (csrc/warp_taps.hip, libvsrlab_warp_taps.so)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _lib
from ._base import _STORAGE_DT, _f32c, _ptr, _require_gpu, _stream, resolve_dtype
from .layout import _pm_dims, _pm_like, from_pixel_major, to_pixel_major


class _FlowWarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow_planar, dtype, border=0):
        n, c, h, w = x.shape
        lib = _lib.load()
        xin = to_pixel_major(x, dtype)
        cp = _pm_dims(xin)[3]
        out = _pm_like(xin)
        flow_planar = _f32c(flow_planar)
        _lib.check(lib.vsr_flow_warp_fwd_ex(dtype, _ptr(xin), _ptr(flow_planar), _ptr(out), n, h, w, cp, border, _stream()), "flow_warp_fwd")
        ctx.save_for_backward(flow_planar, xin if ctx.needs_input_grad[1] else None)
        ctx.meta = (dtype, c, cp, border)
        return from_pixel_major(out, c)

    @staticmethod
    def backward(ctx, gout):
        flow_planar, xin = ctx.saved_tensors
        dtype, c, cp, border = ctx.meta
        n, _, h, w = gout.shape
        lib = _lib.load()
        g = to_pixel_major(gout, dtype, cp)
        gx = gflow = None
        if ctx.needs_input_grad[0]:
            acc = torch.zeros((n, h, w, cp), dtype=torch.float32, device=gout.device)  # plain [N][H][W][C] fp32 accumulator
            _lib.check(lib.vsr_flow_warp_bwd_ex(dtype, _ptr(g), _ptr(flow_planar), _ptr(acc), n, h, w, cp, border, _stream()), "flow_warp_bwd")
            gx = acc[..., :c].permute(0, 3, 1, 2).contiguous()
        if ctx.needs_input_grad[1]:
            gflow = torch.empty((n, 2, h, w), dtype=torch.float32, device=gout.device)
            _lib.check(lib.vsr_flow_warp_bwd_flow_ex(dtype, _ptr(xin), _ptr(g), _ptr(flow_planar), _ptr(gflow), n, h, w, cp, border, _stream()),
                       "flow_warp_bwd_flow")
        return gx, gflow, None, None


def flow_warp(x: torch.Tensor, flow: torch.Tensor, interpolation: str = "bilinear", padding_mode: str = "zeros",
              align_corners: bool = True, compute_dtype: Optional[str] = None) -> torch.Tensor:
    """Drop-in for the reference ``flow_warp(x, flow)``: ``flow`` is channels-last (N,H,W,2),
    [...,0] = horizontal displacement in pixels.  Differentiable w.r.t. ``x`` and ``flow``.

    ``interpolation`` 'nearest' and 'nearest4' (VRT's modes, vsr/models/VRT/modules/spynet.py:39-54) are the integer-tap gathers of
    csrc/warp_taps.hip: ``x`` fp32 or bf16, the result of ``x``'s dtype with C or 4 C channels, bit-identical to
    the reference; the gradient w.r.t. ``x`` is the scatter of the taps and the gradient w.r.t. ``flow`` is zeros.
    ``compute_dtype`` does not apply to them."""
    if interpolation in ("nearest", "nearest4"):
        return _warp_taps(x, flow, 4 if interpolation == "nearest4" else 1, padding_mode, align_corners)
    if interpolation != "bilinear" or padding_mode not in ("zeros", "border") or not align_corners:
        raise NotImplementedError("HIP flow_warp implements the reference's two uses: bilinear, align_corners=True, padding "
                                  "'zeros' (propagation, basicvsr.py:55,70) or 'border' (SPyNet, spynet.py:60)")
    _require_gpu(x, flow)
    return _FlowWarpFn.apply(x, flow.permute(0, 3, 1, 2), resolve_dtype(compute_dtype), 1 if padding_mode == "border" else 0)


# --------------------------------------------------------------------------------------------- #
# integer-tap warps and VRT's aligned input (csrc/warp_taps.hip, libvsrlab_warp_taps.so)
# --------------------------------------------------------------------------------------------- #
def _warp_taps_desc(n, d, c, h, w, taps, border, dtype, x_nstride=0):
    return _lib.WarpTapsDesc(n, d, c, h, w, taps, border, _STORAGE_DT[dtype], x_nstride)


def _warp_taps_checks(x, what):
    if x.dtype not in _STORAGE_DT:
        raise ValueError(f"{what}: x must be float32 or bfloat16; got {x.dtype}")
    if x.shape[-2] < 2 or x.shape[-1] < 2:
        raise NotImplementedError(f"{what}: H and W must be at least 2, got {x.shape[-2]} x {x.shape[-1]} (at extent 1 the reference's "
                                  "max(w - 1, 1) normalisation makes every tap read index 0)")


def _flow_f32(flow: torch.Tensor) -> torch.Tensor:
    return flow if flow.dtype == torch.float32 and flow.is_contiguous() else _f32c(flow)


class _WarpTapsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow_planar, taps, border, save):
        n, c, h, w = (int(v) for v in x.shape)
        # a frame x[:, i] of a clip is read as it lies: dense images, any stride between them
        dense = x.stride()[1:] == (h * w, w, 1) and (n == 1 or x.stride(0) >= c * h * w)
        xin = x.detach() if dense else x.detach().contiguous()
        desc = _warp_taps_desc(n, 1, c, h, w, taps, border, x.dtype, xin.stride(0) if n > 1 else 0)
        flow = _flow_f32(flow_planar.detach())
        out = torch.empty((n, taps * c, h, w), dtype=x.dtype, device=x.device)
        _lib.check(_lib.load_warp_taps().vsr_warp_taps_fwd(ctypes.byref(desc), _ptr(xin), _ptr(flow), _ptr(out), _stream()), "warp_taps_fwd")
        if save:
            ctx.save_for_backward(flow)
        ctx.meta = (n, c, h, w, taps, border, flow_planar.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        n, c, h, w, taps, border, flow_dtype = ctx.meta
        gx = None
        if ctx.needs_input_grad[0]:
            flow, = ctx.saved_tensors
            gout = gout.contiguous()
            desc = _warp_taps_desc(n, 1, c, h, w, taps, border, gout.dtype)
            acc = torch.empty((n, c, h, w), dtype=torch.float32, device=gout.device)
            gx = acc if gout.dtype == torch.float32 else torch.empty_like(acc, dtype=gout.dtype)
            _lib.check(_lib.load_warp_taps().vsr_warp_taps_bwd(ctypes.byref(desc), _ptr(gout), _ptr(flow), _ptr(acc), _ptr(gx), _stream()),
                       "warp_taps_bwd")
        gflow = torch.zeros((n, 2, h, w), dtype=flow_dtype, device=gout.device) if ctx.needs_input_grad[1] else None
        return gx, gflow, None, None, None


def _warp_taps(x, flow, taps, padding_mode, align_corners):
    if padding_mode not in ("zeros", "border") or not align_corners:
        raise NotImplementedError("HIP flow_warp 'nearest' / 'nearest4': align_corners=True with padding 'zeros' or 'border' (what the "
                                  "reference calls, vrt.py:219,226); align_corners=False puts integer taps on rounding ties and cannot be pinned")
    if x.dim() != 4 or flow.dim() != 4 or tuple(flow.shape) != (x.shape[0], x.shape[2], x.shape[3], 2):
        raise ValueError(f"flow_warp: x (N, C, H, W) and flow (N, H, W, 2) expected; got {tuple(x.shape)} and {tuple(flow.shape)}")
    _warp_taps_checks(x, "flow_warp")
    _require_gpu(x, flow)
    # only the gradient w.r.t. x needs anything from the forward (the flow); under no_grad nothing is kept
    return _WarpTapsFn.apply(x, flow.permute(0, 3, 1, 2), taps, 1 if padding_mode == "border" else 0, torch.is_grad_enabled() and x.requires_grad)


class _AlignedInputFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flows_backward, flows_forward, save):
        b, d, c, h, w = (int(v) for v in x.shape)
        desc = _warp_taps_desc(b, d, c, h, w, 4, 0, x.dtype)
        xin = x.detach().contiguous()
        fb, ff = _flow_f32(flows_backward.detach()), _flow_f32(flows_forward.detach())
        out = torch.empty((b, d, 9 * c, h, w), dtype=x.dtype, device=x.device)
        _lib.check(_lib.load_warp_taps().vsr_warp_taps_clip_fwd(ctypes.byref(desc), _ptr(xin), _ptr(fb), _ptr(ff), _ptr(out), _stream()),
                   "warp_taps_clip_fwd")
        if save:
            ctx.save_for_backward(fb, ff)
        ctx.meta = (b, d, c, h, w, flows_backward.dtype, flows_forward.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        b, d, c, h, w, dt_b, dt_f = ctx.meta
        gx = None
        if ctx.needs_input_grad[0]:
            fb, ff = ctx.saved_tensors
            gout = gout.contiguous()
            desc = _warp_taps_desc(b, d, c, h, w, 4, 0, gout.dtype)
            acc = torch.empty((b, d, c, h, w), dtype=torch.float32, device=gout.device)
            gx = acc if gout.dtype == torch.float32 else torch.empty_like(acc, dtype=gout.dtype)
            _lib.check(_lib.load_warp_taps().vsr_warp_taps_clip_bwd(ctypes.byref(desc), _ptr(gout), _ptr(fb), _ptr(ff), _ptr(acc), _ptr(gx),
                                                                    _stream()), "warp_taps_clip_bwd")
        mk = lambda need, dt: torch.zeros((b, d - 1, 2, h, w), dtype=dt, device=gout.device) if need else None
        return gx, mk(ctx.needs_input_grad[1], dt_b), mk(ctx.needs_input_grad[2], dt_f), None


def aligned_input(x: torch.Tensor, flows_backward: torch.Tensor, flows_forward: torch.Tensor) -> torch.Tensor:
    """``cat([x, x_backward, x_forward], 2)`` of VRT.forward (vrt.py:149-150) in one launch: ``x`` (B, D, C, H, W) fp32 or bf16,
    both flows (B, D - 1, 2, H, W) -> (B, D, 9 C, H, W), where ``x_backward`` / ``x_forward`` are what ``get_aligned_image`` stacks
    from its 'nearest4' warps and zero blocks.  The kernel writes the copy of ``x`` and the zero blocks too.  Differentiable w.r.t.
    ``x``; the flows get zeros."""
    if x.dim() != 5 or x.shape[1] < 2:
        raise ValueError(f"aligned_input: x must be (B, D, C, H, W) with D >= 2; got {tuple(x.shape)}")
    b, d, c, h, w = x.shape
    for name, f in (("flows_backward", flows_backward), ("flows_forward", flows_forward)):
        if tuple(f.shape) != (b, d - 1, 2, h, w):
            raise ValueError(f"aligned_input: {name} must be {(b, d - 1, 2, h, w)}; got {tuple(f.shape)}")
    _warp_taps_checks(x, "aligned_input")
    _require_gpu(x, flows_backward, flows_forward)
    return _AlignedInputFn.apply(x, flows_backward, flows_forward, torch.is_grad_enabled() and x.requires_grad)
