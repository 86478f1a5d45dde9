"""SPyNet on the HIP engine (reference: vsr/models/RealBasicVSR/modules/spynet.py:69-93 and the canonical
vsr/models/VRT/modules/spynet.py:68-157; csrc/spynet_engine.hip), and SpynetModule as single conv layers."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .. import _lib
from ._base import _f32c, _ptr, _ptr_array, _require_gpu, _stream, resolve_dtype
from .conv import _conv_layer_autograd


class _SpynetFn(torch.autograd.Function):
    """flow = Spynet(ref, supp) with its backward on the HIP engine: parameter gradients (train_flow) and the gradient
    w.r.t. the two frames (border warps, image pyramid, /32 resize, normalisation)."""

    @staticmethod
    def forward(ctx, ref, supp, dtype, need_bwd, *params):
        n, _, h, w = ref.shape
        lib = _lib.load()
        ps = [_f32c(p) for p in params]
        ws = torch.empty(lib.vsr_spynet_workspace_bytes(n, h, w, dtype, int(need_bwd)), dtype=torch.uint8, device=ref.device)
        flow = torch.empty((n, 2, h, w), dtype=torch.float32, device=ref.device)
        _lib.check(lib.vsr_spynet_forward(n, h, w, dtype, _ptr_array(ps), len(ps), _ptr(_f32c(ref)), _ptr(_f32c(supp)), _ptr(flow),
                                          _ptr(ws), ws.numel(), int(need_bwd), _stream()), "spynet_forward")
        ctx.meta = (n, h, w, dtype, need_bwd)
        ctx.ws = ws if need_bwd else None
        ctx.ps = ps
        return flow

    @staticmethod
    def backward(ctx, dflow):
        n, h, w, dtype, need_bwd = ctx.meta
        if not need_bwd:
            raise RuntimeError("vsrlab_amd: backward through a SPyNet forward that ran without need_backward")
        if ctx.ws is None:
            raise RuntimeError("vsrlab_amd: trying to backward through the SPyNet graph a second time")
        lib = _lib.load()
        want_p = any(ctx.needs_input_grad[4 + k] for k in range(60))
        grads = [torch.zeros_like(p) if (k < 60 and want_p) else None for k, p in enumerate(ctx.ps)]
        dref = torch.empty((n, 3, h, w), dtype=torch.float32, device=dflow.device) if ctx.needs_input_grad[0] else None
        dsupp = torch.empty((n, 3, h, w), dtype=torch.float32, device=dflow.device) if ctx.needs_input_grad[1] else None
        _lib.check(lib.vsr_spynet_backward_ex(n, h, w, dtype, _ptr_array(ctx.ps), _ptr_array(grads) if want_p else None, len(grads),
                                              _ptr(_f32c(dflow)), 1, None, _ptr(dref), _ptr(dsupp), _ptr(ctx.ws), ctx.ws.numel(), _stream()),
                   "spynet_backward")
        ctx.ws = None
        return (dref, dsupp, None, None) + tuple(g if (g is not None and ctx.needs_input_grad[4 + k]) else None
                                                 for k, g in enumerate(grads))


def spynet_flow(params: Sequence[torch.Tensor], ref: torch.Tensor, supp: torch.Tensor,
                compute_dtype: Optional[str] = None) -> torch.Tensor:
    """``params``: the 62 Spynet tensors in state_dict order (60 conv tensors, mean, std).  Differentiable w.r.t. the
    60 conv tensors (train_flow, basicvsr.py:25-28) and w.r.t. both frames."""
    _require_gpu(ref, supp)
    if len(params) != 62:
        raise ValueError("expected the 62 tensors of Spynet.state_dict()")
    need_bwd = torch.is_grad_enabled() and (ref.requires_grad or supp.requires_grad or any(p.requires_grad for p in params[:60]))
    return _SpynetFn.apply(ref, supp, resolve_dtype(compute_dtype), need_bwd, *params)


class _SpynetLevelsFn(torch.autograd.Function):
    """The per-level flows of the canonical SPyNet with their backward on the HIP engine (vsr_spynet_forward_ex /
    vsr_spynet_backward_ex): parameter gradients and the gradient w.r.t. both frames, from the cotangents of every returned
    level (vsr/models/VRT/modules/spynet.py:98-157 under autograd)."""

    @staticmethod
    def forward(ctx, ref, supp, dtype, need_bwd, last_relu, levels, *params):
        n, _, h, w = ref.shape
        lib = _lib.load()
        ps = [_f32c(p) for p in params]
        ws = torch.empty(lib.vsr_spynet_workspace_bytes(n, h, w, dtype, int(need_bwd)), dtype=torch.uint8, device=ref.device)
        outs: List[Optional[torch.Tensor]] = [None] * 6
        for lv in levels:
            outs[lv] = torch.empty((n, 2, h >> (5 - lv), w >> (5 - lv)), dtype=torch.float32, device=ref.device)
        _lib.check(lib.vsr_spynet_forward_ex(n, h, w, dtype, _ptr_array(ps), len(ps), _ptr(_f32c(ref)), _ptr(_f32c(supp)), int(last_relu),
                                             _ptr_array(outs), _ptr(ws), ws.numel(), int(need_bwd), _stream()), "spynet_forward_ex")
        ctx.meta = (n, h, w, dtype, need_bwd, last_relu, levels)
        ctx.ws = ws if need_bwd else None
        ctx.ps = ps
        return tuple(outs[lv] for lv in levels)

    @staticmethod
    def backward(ctx, *douts):
        n, h, w, dtype, need_bwd, last_relu, levels = ctx.meta
        if not need_bwd:
            raise RuntimeError("vsrlab_amd: backward through a SPyNet forward that ran without need_backward")
        if ctx.ws is None:
            raise RuntimeError("vsrlab_amd: trying to backward through the SPyNet graph a second time")
        lib = _lib.load()
        dlevel: List[Optional[torch.Tensor]] = [None] * 6
        for lv, d in zip(levels, douts):
            if d is not None:
                dlevel[lv] = _f32c(d)
        want_p = any(ctx.needs_input_grad[6 + k] for k in range(60))
        grads = [torch.zeros_like(p) if (k < 60 and want_p) else None for k, p in enumerate(ctx.ps)]
        dev = ctx.ps[0].device
        dref = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dsupp = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if all(d is None for d in dlevel):
            if dref is not None:
                dref.zero_()
            if dsupp is not None:
                dsupp.zero_()
        else:
            _lib.check(lib.vsr_spynet_backward_ex(n, h, w, dtype, _ptr_array(ctx.ps), _ptr_array(grads) if want_p else None, len(grads),
                                                  None, int(last_relu), _ptr_array(dlevel), _ptr(dref), _ptr(dsupp), _ptr(ctx.ws),
                                                  ctx.ws.numel(), _stream()), "spynet_backward")
        ctx.ws = None
        return (dref, dsupp, None, None, None, None) + tuple(g if (g is not None and ctx.needs_input_grad[6 + k]) else None
                                                             for k, g in enumerate(grads))


def spynet_levels(params: Sequence[torch.Tensor], ref: torch.Tensor, supp: torch.Tensor, return_levels: Sequence[int],
                  last_relu: bool = False, compute_dtype: Optional[str] = None) -> List[torch.Tensor]:
    """The canonical SPyNet (vsr/models/VRT/modules/spynet.py:68-157): the flows of the requested pyramid levels (5 = full
    resolution, 4 = 1/2, ...), finest first, like the reference's ``flow_list``; differentiable w.r.t. the 60 conv tensors
    and both frames."""
    _require_gpu(ref, supp)
    if len(params) != 62:
        raise ValueError("expected the 62 tensors of SpyNet.state_dict()")
    levels = tuple(sorted(set(int(v) for v in return_levels), reverse=True))
    if not levels or not all(0 <= lv <= 5 for lv in levels):
        raise ValueError("return_levels are pyramid levels 0..5")
    need_bwd = torch.is_grad_enabled() and (ref.requires_grad or supp.requires_grad or any(p.requires_grad for p in params[:60]))
    return list(_SpynetLevelsFn.apply(ref, supp, resolve_dtype(compute_dtype), need_bwd, bool(last_relu), levels, *params))


def spynet_module_forward(x: torch.Tensor, params: Sequence[torch.Tensor], last_relu: bool = True,
                          compute_dtype: Optional[str] = None) -> torch.Tensor:
    """SpynetModule.forward (spynet.py:13-21): (N,8,h,w) -> (N,2,h,w) through the five 7x7 layers; differentiable w.r.t. x and
    the ten parameter tensors."""
    _require_gpu(x)
    if x.shape[1] != 8 or len(params) != 10:
        raise ValueError("SpynetModule takes (N,8,h,w) and has 10 parameter tensors")
    y = x
    for j in range(4):
        y = _conv_layer_autograd(y, None, params[2 * j], params[2 * j + 1], 1, compute_dtype=compute_dtype)
    return _conv_layer_autograd(y, None, params[8], params[9], 1 if last_relu else 0, planar_out=True, compute_dtype=compute_dtype)
