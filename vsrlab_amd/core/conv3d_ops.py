"""The torch-facing entry of ``libvsrlab_conv3d.so`` (``csrc/conv3d.hip``, ``include/vsrlab_conv3d.h``): the stride-1 'same' Conv3d with
(1,3,3), (3,1,1) or (3,3,3) taps behind ``core.modules.conv.ConvST`` / ``ConvSTBlock``, ``core.modules.upsampling.PixelShufflePack3D``
and VRT's ``Upsample``.  DESIGN section 11k.

It lives here, beside its users, and not in ``vsrlab_amd.functional``, whose set of names is pinned.  PyTorch supplies device memory,
the current stream and the autograd bookkeeping; there is no CPU / eager fallback: a tensor that is not on a GPU raises.  Activations
are fp32 or bf16 and read where they lie, through their strides (any other dtype goes through fp32); weights and biases are fp32."""
from __future__ import annotations

import ctypes

import torch

from .. import _lib
from ..functional import _STORAGE_DT, _ptr, _require_gpu, _stream

TAP_SETS = {(1, 3, 3): _lib.CONV3D_133, (3, 1, 1): _lib.CONV3D_311, (3, 3, 3): _lib.CONV3D_333}
MAX_CHANNELS = _lib.CONV3D_MAX_C
_ACTS = {None: _lib.CONV3D_ACT_NONE, "leaky_relu": _lib.CONV3D_ACT_LEAKY}


def _no_double_backward() -> None:
    if torch.is_grad_enabled():
        raise RuntimeError("vsrlab_amd: conv3d has no double backward (create_graph=True is not supported)")


def _bct(t: torch.Tensor, time_major: bool) -> torch.Tensor:
    """the (b, c, t, h, w) view of a tensor in either axis order"""
    return t.transpose(1, 2) if time_major else t


def _readable(v: torch.Tensor) -> torch.Tensor:
    """A (b, c, t, h, w) view as the kernels read it: the H x W planes contiguous and no two elements on one address (so that the
    gradient can be written through the same strides); anything else is copied."""
    B, C, T, H, W = v.shape
    ok = (W == 1 or v.stride(4) == 1) and (H == 1 or v.stride(3) == W)
    need = H * W
    for size, stride in sorted(((v.size(i), v.stride(i)) for i in range(3) if v.size(i) > 1), key=lambda p: p[1]):
        ok = ok and stride >= need
        need = stride * size
    return v if ok else v.contiguous()


def _like_order(v: torch.Tensor, C: int, H: int, W: int) -> torch.Tensor:
    """an uninitialised (b, C, t, H, W) tensor whose batch, channel and frame axes lie in memory in the order of v's"""
    sizes = [v.size(0), C, v.size(2)]
    order = sorted(range(3), key=lambda i: (-v.stride(i), i))
    out = torch.empty([sizes[i] for i in order] + [H, W], dtype=v.dtype, device=v.device)
    inv = [order.index(i) for i in range(3)]
    return out.permute(*inv, 3, 4)


def _desc(xv, yv, Cout, taps, act, slope, shuffle):
    B, Cin, T, H, W = xv.shape
    d = _lib.Conv3dDesc(B, Cin, Cout, T, H, W, taps, _STORAGE_DT[xv.dtype], act, float(slope), shuffle)
    for i in range(3):
        d.x_stride[i] = xv.stride(i)
        d.y_stride[i] = yv.stride(i)
    return d


def _workspace(desc, backward, device):
    n = _lib.load_conv3d().vsr_conv3d_workspace_bytes(ctypes.byref(desc), 1 if backward else 0)
    if n == 0:
        raise RuntimeError("vsrlab_amd: conv3d: the shape is outside what the kernels cover (channels <= "
                           f"{MAX_CHANNELS}, offsets below 2^62)")
    return torch.empty(n, dtype=torch.uint8, device=device), n


class _Conv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, taps, act, slope, shuffle, time_major):
        xs = x.detach()
        if xs.dtype not in _STORAGE_DT:
            xs = xs.to(torch.float32)
        xv = _readable(_bct(xs, time_major))
        ws = weight.detach().to(torch.float32).contiguous()
        bs = None if bias is None else bias.detach().to(torch.float32).contiguous()
        Cout, H, W = ws.shape[0], xv.size(3), xv.size(4)
        yv = _like_order(xv, Cout // 4, 2 * H, 2 * W) if shuffle else _like_order(xv, Cout, H, W)
        desc = _desc(xv, yv, Cout, taps, act, slope, shuffle)
        work, n = _workspace(desc, False, xv.device)
        _lib.check(_lib.load_conv3d().vsr_conv3d_fwd(ctypes.byref(desc), _ptr(xv), _ptr(ws), _ptr(bs), _ptr(yv), _ptr(work), n, _stream()),
                   "conv3d_fwd")
        ctx.cfg = (Cout, taps, act, slope, shuffle, time_major, x.dtype, weight.dtype, None if bias is None else bias.dtype)
        ctx.save_for_backward(xv, ws, yv if act != _lib.CONV3D_ACT_NONE else None)
        ctx.y_stride = yv.stride()
        return _bct(yv, time_major).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        _no_double_backward()
        xv, ws, yv = ctx.saved_tensors
        Cout, taps, act, slope, shuffle, time_major, x_dtype, w_dtype, b_dtype = ctx.cfg
        gv = _bct(g.detach().to(xv.dtype), time_major)
        if gv.stride() != ctx.y_stride:                       # the cotangent through y's strides
            gy = torch.empty_strided(gv.shape, ctx.y_stride, dtype=gv.dtype, device=gv.device)
            gy.copy_(gv)
            gv = gy
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], b_dtype is not None and ctx.needs_input_grad[2]
        dx = torch.empty_strided(xv.shape, xv.stride(), dtype=xv.dtype, device=xv.device) if need_x else None
        dw = torch.empty_like(ws) if need_w else None
        db = torch.empty(Cout, dtype=torch.float32, device=xv.device) if need_b else None
        desc = _desc(xv, gv, Cout, taps, act, slope, shuffle)
        work, n = _workspace(desc, True, xv.device)
        _lib.check(_lib.load_conv3d().vsr_conv3d_bwd(ctypes.byref(desc), _ptr(xv), _ptr(ws), _ptr(yv), _ptr(gv), _ptr(dx), _ptr(dw), _ptr(db),
                                                     _ptr(work), n, _stream()), "conv3d_bwd")
        return (None if dx is None else _bct(dx, time_major).to(x_dtype), None if dw is None else dw.to(w_dtype),
                None if db is None else db.to(b_dtype), None, None, None, None, None)


def conv3d(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None, slope: float = 0.01,
           pixel_shuffle: int = 0, time_major: bool = False) -> torch.Tensor:
    """``act(F.conv3d(x, weight, bias, stride=1, padding=k // 2))`` in one launch, differentiable w.r.t. ``x``, ``weight`` and ``bias``.

    ``x``: (b, c, t, h, w), or (b, t, c, h, w) with ``time_major`` -- fp32 or bf16, and a view is accepted: its batch, channel and
    frame strides go into the descriptor, and it is copied only when an h x w plane itself is not contiguous (or two of its elements
    share an address).  ``weight``: (Cout, Cin, kt, kh, kw) with (kt, kh, kw) one of (1,3,3), (3,1,1), (3,3,3).  ``act``: None or
    'leaky_relu' (``slope`` > 0).  ``pixel_shuffle`` = 2: the result is (.., Cout / 4, .., 2h, 2w), ``nn.PixelShuffle(2)`` on the last
    three axes of the (b, t, c, h, w) order, as the store pattern.  The result has x's dtype, axis order and memory order."""
    _require_gpu(x, weight, *(() if bias is None else (bias,)))
    if x.dim() != 5 or weight.dim() != 5:
        raise ValueError(f"conv3d takes a 5-D input and weight, got {tuple(x.shape)} and {tuple(weight.shape)}")
    k = tuple(weight.shape[2:])
    if k not in TAP_SETS:
        raise NotImplementedError(f"conv3d: kernel {k} is not one of {sorted(TAP_SETS)}")
    if act not in _ACTS:
        raise ValueError(f"conv3d: act {act!r} is not one of {list(_ACTS)}")
    if pixel_shuffle not in (0, 2):
        raise NotImplementedError(f"conv3d: pixel_shuffle {pixel_shuffle} is not 0 or 2")
    Cout, Cin = weight.shape[:2]
    if x.size(2 if time_major else 1) != Cin:
        raise ValueError(f"conv3d: the input {tuple(x.shape)} has not the weight's {Cin} channels")
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError(f"conv3d: the bias {tuple(bias.shape)} is not ({Cout},)")
    if pixel_shuffle and Cout % 4:
        raise ValueError(f"conv3d: pixel_shuffle = 2 needs a multiple of 4 output channels, got {Cout}")
    if max(Cin, Cout) > MAX_CHANNELS:
        raise NotImplementedError(f"conv3d: {Cin} -> {Cout} channels, the kernels cover up to {MAX_CHANNELS}")
    if act is not None and not slope > 0:
        raise ValueError(f"conv3d: the LeakyReLU slope must be positive (the backward reads the sign off the output), got {slope}")
    if x.numel() == 0:
        raise ValueError(f"conv3d: empty input {tuple(x.shape)}")
    return _Conv3dFn.apply(x, weight, bias, TAP_SETS[k], _ACTS[act], float(slope), int(pixel_shuffle), bool(time_major))
