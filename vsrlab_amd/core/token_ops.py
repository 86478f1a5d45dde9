"""The torch-facing entries of ``libvsrlab_mixer.so`` (``csrc/token_mixer.hip``, ``include/vsrlab_mixer.h``): the block transform
behind ``core.modules.dct_transforms`` and the residual MLP along one axis behind ``core.modules.mlp``.  DESIGN section 11j.

They live here, beside their users, and not in ``vsrlab_amd.functional``, whose set of names is pinned.  PyTorch supplies device
memory, the current stream and the autograd bookkeeping; there is no CPU / eager fallback: a tensor that is not on a GPU raises.
Activations are fp32 or bf16 and read where they lie (any other dtype goes through fp32); weights and biases are fp32."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib
from ..functional import _STORAGE_DT, _ptr, _require_gpu, _stream

BLOCK_SIZES = (2, 4, 8)
MAX_TOKEN_CHANNELS = 256


def _activation(t: torch.Tensor) -> torch.Tensor:
    """The tensor as the kernels read it: fp32 and bf16 where they lie, any other dtype as fp32; dense."""
    t = t.detach()
    if t.dtype not in _STORAGE_DT:
        t = t.to(torch.float32)
    return t.contiguous()


def _weight(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _no_double_backward(name: str) -> None:
    if torch.is_grad_enabled():
        raise RuntimeError(f"vsrlab_amd: {name} has no double backward (create_graph=True is not supported)")


# ---- block transform -------------------------------------------------------------------------------------------------------------
def _dct_desc(N, C, H, W, ps, dtype):
    return _lib.BlockDctDesc(N, C, H, W, ps, _STORAGE_DT[dtype])


def _run_dct(x: torch.Tensor, w: torch.Tensor, ps: int) -> torch.Tensor:
    """planar (N, C, H, W) -> tokens (N, P, C ps^2)"""
    N, C, H, W = x.shape
    y = torch.empty(N, (H // ps) * (W // ps), C * ps * ps, dtype=x.dtype, device=x.device)
    desc = _dct_desc(N, C, H, W, ps, x.dtype)
    _lib.check(_lib.load_mixer().vsr_block_dct_fwd(ctypes.byref(desc), _ptr(x), _ptr(w), _ptr(y), _stream()), "block_dct")
    return y


def _run_idct(y: torch.Tensor, w: torch.Tensor, ps: int, C: int, H: int, W: int) -> torch.Tensor:
    """tokens (N, P, C ps^2) -> planar (N, C, H, W), the remainder rows and columns zero"""
    N = y.shape[0]
    x = torch.empty(N, C, H, W, dtype=y.dtype, device=y.device)
    desc = _dct_desc(N, C, H, W, ps, y.dtype)
    _lib.check(_lib.load_mixer().vsr_block_idct_fwd(ctypes.byref(desc), _ptr(y), _ptr(w), _ptr(x), _stream()), "block_idct")
    return x


class _BlockDctFn(torch.autograd.Function):
    """Each kernel is the other's adjoint for the same weight: the backward of one is the other."""

    @staticmethod
    def forward(ctx, x, w, ps, inverse, C, H, W):
        xs, ws = _activation(x), _weight(w)
        ctx.ps, ctx.inverse, ctx.dtype = ps, inverse, x.dtype
        ctx.save_for_backward(ws)
        if inverse:
            return _run_idct(xs, ws, ps, C, H, W).to(x.dtype)
        ctx.chw = tuple(xs.shape[1:])
        return _run_dct(xs, ws, ps).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        _no_double_backward("block_idct" if ctx.inverse else "block_dct")
        (ws,) = ctx.saved_tensors
        gs = _activation(g)
        gx = _run_dct(gs, ws, ctx.ps) if ctx.inverse else _run_idct(gs, ws, ctx.ps, *ctx.chw)
        return gx.to(ctx.dtype), None, None, None, None, None, None


def _check_block_args(name: str, w: torch.Tensor, ps: int, C: int) -> None:
    if ps not in BLOCK_SIZES:
        raise ValueError(f"{name}: block size {ps} is not one of {BLOCK_SIZES}")
    if C * ps * ps > MAX_TOKEN_CHANNELS:
        raise ValueError(f"{name}: {C} channels of {ps} x {ps} blocks make tokens of {C * ps * ps} > {MAX_TOKEN_CHANNELS} values")
    if w.requires_grad:
        raise RuntimeError(f"{name}: the transform's weight is frozen (requires_grad = False in the reference): there is no weight gradient")
    if w.numel() != C * ps ** 4:
        raise ValueError(f"{name}: the weight has {w.numel()} elements, ({C * ps * ps}, 1, {ps}, {ps}) has {C * ps ** 4}")


def block_dct(x: torch.Tensor, w: torch.Tensor, ps: int) -> torch.Tensor:
    """``F.conv2d(x, w, stride=ps, groups=C)`` as tokens: ``x`` (N, C, H, W) -> (N, (H // ps)(W // ps), C ps^2), token
    ``bi (W // ps) + bj``, differentiable w.r.t. ``x``.  ``w``: (C ps^2, 1, ps, ps), frozen.  Rows and columns past the last whole
    block are ignored, as the convolution ignores them."""
    _require_gpu(x, w)
    if x.dim() != 4:
        raise ValueError(f"block_dct takes (N, C, H, W), got {tuple(x.shape)}")
    N, C, H, W = x.shape
    _check_block_args("block_dct", w, ps, C)
    if N < 1 or H < ps or W < ps:
        raise ValueError(f"block_dct: {tuple(x.shape)} holds no {ps} x {ps} block")
    return _BlockDctFn.apply(x, w, ps, False, C, H, W)


def block_idct(tokens: torch.Tensor, w: torch.Tensor, ps: int, H: int, W: int) -> torch.Tensor:
    """``F.conv_transpose2d(.., w, stride=ps, groups=C)`` from tokens: (N, (H // ps)(W // ps), C ps^2) -> (N, C, H, W), the rows and
    columns past the last whole block zero; differentiable w.r.t. ``tokens``.  The adjoint of ``block_dct`` for the same ``w``."""
    _require_gpu(tokens, w)
    if tokens.dim() != 3:
        raise ValueError(f"block_idct takes (N, P, C ps^2), got {tuple(tokens.shape)}")
    N, P, CK = tokens.shape
    if CK % (ps * ps):
        raise ValueError(f"block_idct: tokens of {CK} values are no whole number of {ps} x {ps} blocks")
    C = CK // (ps * ps)
    _check_block_args("block_idct", w, ps, C)
    if N < 1 or H < ps or W < ps or P != (H // ps) * (W // ps):
        raise ValueError(f"block_idct: {P} tokens do not tile ({H}, {W}) in {ps} x {ps} blocks: that takes {(H // ps) * (W // ps)}")
    return _BlockDctFn.apply(tokens, w, ps, True, C, H, W)


# ---- residual MLP along one axis ---------------------------------------------------------------------------------------------------
def _mlp_desc(outer, D, inner, hidden, dtype=torch.float32, residual=True):
    return _lib.AxisMlpDesc(outer, D, inner, hidden, _STORAGE_DT[dtype], int(residual))


def axis_mlp_is_fused(D: int, hidden: int) -> bool:
    """Whether an axis of length ``D`` with ``hidden`` hidden units runs on the fused kernel (``vsr_axis_mlp_supported``) or, past its
    bound, on the batched-matmul path of ``axis_mlp``."""
    desc = _mlp_desc(1, D, 1, hidden)
    return bool(_lib.load_mixer().vsr_axis_mlp_supported(ctypes.byref(desc)))


class _AxisMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, view, residual):
        outer, D, inner = view
        xs = _activation(x)
        ws = tuple(_weight(t) for t in (w1, b1, w2, b2))
        y = torch.empty_like(xs)
        desc = _mlp_desc(outer, D, inner, ws[0].shape[0], xs.dtype, residual)
        _lib.check(_lib.load_mixer().vsr_axis_mlp_fwd(ctypes.byref(desc), _ptr(xs), *(_ptr(t) for t in ws), _ptr(y), _stream()), "axis_mlp")
        ctx.view, ctx.residual, ctx.dtype = view, residual, x.dtype
        ctx.save_for_backward(xs, *ws)                      # the hidden vector is recomputed: no activation is kept
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        _no_double_backward("axis_mlp")
        xs, *ws = ctx.saved_tensors
        outer, D, inner = ctx.view
        lib = _lib.load_mixer()
        gs = _activation(g)
        if gs.dtype != xs.dtype:
            gs = gs.to(xs.dtype)
        desc = _mlp_desc(outer, D, inner, ws[0].shape[0], xs.dtype, ctx.residual)
        dx = torch.empty_like(xs) if ctx.needs_input_grad[0] else None
        grads, scratch, nbytes = (None,) * 4, None, 0
        if any(ctx.needs_input_grad[1:5]):
            grads = tuple(torch.empty_like(t) for t in ws)
            nbytes = lib.vsr_axis_mlp_scratch_bytes(ctypes.byref(desc))
            scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=xs.device)
        _lib.check(lib.vsr_axis_mlp_bwd(ctypes.byref(desc), _ptr(xs), _ptr(gs), *(_ptr(t) for t in ws), _ptr(dx), *(_ptr(t) for t in grads),
                                        _ptr(scratch), nbytes, _stream()), "axis_mlp_bwd")
        return (None if dx is None else dx.to(ctx.dtype),
                *(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[1:5])), None, None)


def _axis_mlp_matmul(x, view, w1, b1, w2, b2, residual):
    """Past the fused kernel's bound the MLP is a real GEMM: torch's batched matmul on the (outer, D, inner) view, W1 @ X per
    ``outer`` index, which needs no permute copy; autograd is torch's.  GEMM plumbing, not a fallback for a missing kernel."""
    outer, D, inner = view
    X = x.reshape(outer, D, inner).to(torch.float32)        # fp32 arithmetic, as on the fused path; x's dtype is storage only
    h = torch.matmul(w1.to(torch.float32), X) + b1.to(torch.float32)[:, None]
    m = torch.matmul(w2.to(torch.float32), torch.nn.functional.gelu(h)) + b2.to(torch.float32)[:, None]
    return ((X + m) if residual else m).reshape(x.shape).to(x.dtype)


def axis_mlp(x: torch.Tensor, axis: int, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, residual: bool = True):
    """``x + W2 gelu(W1 x + b1) + b2`` along ``axis`` of a dense tensor (``residual=False``: without the ``x +``), in x's layout: no
    permute is materialised.  ``w1``: (hidden, D), ``w2``: (D, hidden), ``nn.Linear``'s layout; exact (erf) GELU.  Differentiable
    w.r.t. everything; the weight gradients are summed in a fixed order.

    Shapes inside ``axis_mlp_is_fused`` run on the fused HIP kernel.  Beyond it -- a patch axis of hundreds of tokens -- the MLP is a
    real GEMM and runs as torch's batched matmul on the same (outer, D, inner) view of the same GPU tensor: that is GEMM plumbing,
    not a fallback for a missing kernel, and it is never taken for a shape the kernel supports."""
    _require_gpu(x, w1, b1, w2, b2)
    axis = axis % x.dim() if x.dim() else 0
    if x.dim() < 1 or x.numel() < 1:
        raise ValueError("axis_mlp needs at least one element")
    D = x.shape[axis]
    hidden = w1.shape[0]
    if tuple(w1.shape) != (hidden, D) or tuple(b1.shape) != (hidden,) or tuple(w2.shape) != (D, hidden) or tuple(b2.shape) != (D,):
        raise ValueError(f"axis_mlp along an axis of {D}: weights ({hidden}, {D}), ({hidden},), ({D}, {hidden}), ({D},) expected, got "
                         f"{tuple(w1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(b2.shape)}")
    outer = 1
    for s in x.shape[:axis]:
        outer *= s
    view = (outer, D, x.numel() // (outer * D))
    if not axis_mlp_is_fused(D, hidden):
        return _axis_mlp_matmul(x.contiguous(), view, w1, b1, w2, b2, residual)
    return _AxisMlpFn.apply(x, w1, b1, w2, b2, view, residual)
