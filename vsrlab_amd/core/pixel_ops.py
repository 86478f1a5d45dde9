"""The torch-facing entries of ``libvsrlab_losses.so`` (``csrc/pixel_losses.hip``, ``include/vsrlab_losses.h``): the mean L1 and
root-mean-square reductions behind ``core.losses.WL1Loss`` / ``rmse_loss``, fused with their gradient, and the adjoint of the
bilinear resize behind ``core.utils.resize``.  DESIGN section 11i.

They live here, beside their users, and not in ``vsrlab_amd.functional``, whose set of names is pinned.  PyTorch supplies device
memory, the current stream and the autograd bookkeeping; there is no CPU / eager fallback: a tensor that is not on a GPU raises."""
from __future__ import annotations

import torch

from .. import _lib
from ..functional import _STORAGE_DT, _ptr, _require_gpu, _stream


def _operand(t: torch.Tensor) -> torch.Tensor:
    """The tensor as the kernel reads it: fp32 and bf16 where they lie (no fp32 staging copy), any other dtype as fp32; dense."""
    t = t.detach()
    if t.dtype not in _STORAGE_DT:
        t = t.to(torch.float32)
    return t.contiguous()


class _PairLossFn(torch.autograd.Function):
    """``mean |x - y|`` (kind L1) or ``sqrt(mean (x - y)^2)`` (kind MSE with ``root``): value and, when an argument needs one, the
    gradient w.r.t. ``x`` from the same pass over the operands.  The square root and its ``1 / rmse`` factor act on the scalar."""

    @staticmethod
    def forward(ctx, x, y, kind, root, need_grad):
        lib = _lib.load_losses()
        xs, ys = _operand(x), _operand(y)
        dx = torch.empty_like(xs) if need_grad else None
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.vsr_pixel_loss_scratch_floats(), dtype=torch.float32, device=x.device)
        _lib.check(lib.vsr_pixel_loss_fwd_bwd(kind, _ptr(xs), _STORAGE_DT[xs.dtype], _ptr(ys), _STORAGE_DT[ys.dtype], _ptr(dx), _ptr(loss),
                                              _ptr(scratch), xs.numel(), _stream()), "pixel_loss")
        if root:
            loss = torch.sqrt(loss)
        ctx.root, ctx.has_grad = root, need_grad
        ctx.x_dtype, ctx.y_dtype = x.dtype, y.dtype
        ctx.save_for_backward(dx, loss if root else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        name = "rmse_loss" if ctx.root else "l1_loss"
        if torch.is_grad_enabled():
            raise RuntimeError(f"vsrlab_amd: {name} has no double backward (create_graph=True is not supported)")
        if not ctx.has_grad:
            raise RuntimeError(f"vsrlab_amd: backward through a {name} that ran without a gradient")
        dx, rmse = ctx.saved_tensors
        # the scaling pass, in fp32 whatever dx is stored as (a bf16 dx times a 0-dim fp32 tensor would round the FACTOR to bf16 first)
        coef = (g / rmse if ctx.root else g).to(torch.float32)        # x == y everywhere: 0 * (g / 0) = NaN, as in torch
        gx = (dx.to(torch.float32) * coef).to(dx.dtype)
        return (gx.to(ctx.x_dtype) if ctx.needs_input_grad[0] else None,
                (-gx).to(ctx.y_dtype) if ctx.needs_input_grad[1] else None, None, None, None)


def _pair_loss(x: torch.Tensor, y: torch.Tensor, kind: int, root: bool) -> torch.Tensor:
    _require_gpu(x, y)
    if x.shape != y.shape:
        raise ValueError(f"HIP pixel losses take operands of one shape (no broadcasting): got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.numel() < 1:
        raise ValueError("HIP pixel losses need at least one element")
    need_grad = torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)
    return _PairLossFn.apply(x, y, kind, root, need_grad)


def l1_loss(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``F.l1_loss(x, y)`` (mean reduction), differentiable w.r.t. both arguments; ``sign(0) = 0`` in the gradient, as in torch."""
    return _pair_loss(x, y, _lib.LOSS_L1, False)


def rmse_loss(yhat: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``torch.sqrt(torch.mean((yhat - y) ** 2))``, differentiable w.r.t. both arguments.  No epsilon: equal operands give the value 0
    and a NaN gradient, as in torch."""
    return _pair_loss(yhat, y, _lib.LOSS_MSE, True)


def resize_bilinear_backward(gout: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The adjoint of ``vsr_resize_bilinear``: ``gout`` (..., h, w) -> the fp32 gradient (..., H, W) w.r.t. the resized images."""
    _require_gpu(gout)
    h, w = gout.shape[-2:]
    g32 = gout.detach().to(torch.float32).contiguous()
    gin = torch.empty(gout.shape[:-2] + (H, W), dtype=torch.float32, device=gout.device)
    planes = g32.numel() // (h * w)
    _lib.check(_lib.load_losses().vsr_resize_bilinear_bwd(_ptr(g32), _ptr(gin), planes, H, W, h, w, _stream()), "resize_bilinear_bwd")
    return gin
