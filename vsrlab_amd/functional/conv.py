"""The 64-channel conv3x3 pieces and the trunk chain (reference: core/modules/conv.py:82-92; csrc/conv3x3_chain.hip), then the single conv
layers of the reference's building blocks (vsr_conv_layer_fwd / _bwd).  The per-op entries are in csrc/layer_ops.hip."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import DT_BF16, DT_F32
from ._base import MID_CHANNELS, _TORCH_DT, _check_width, _f32c, _ptr, _require_gpu, _stream, resolve_dtype
from .layout import _pm_dims, _pm_like, from_pixel_major, to_pixel_major


def conv3x3_c64(x_pm: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
                res_pm: Optional[torch.Tensor] = None) -> torch.Tensor:
    _require_gpu(x_pm, weight)
    n, h, w, c = _pm_dims(x_pm)
    assert c == 64 and tuple(weight.shape) == (64, 64, 3, 3)
    dtype = DT_BF16 if x_pm.dtype == torch.bfloat16 else DT_F32
    lib = _lib.load()
    wpack = torch.empty(9 * 64 * 64, dtype=x_pm.dtype, device=x_pm.device)
    y = _pm_like(x_pm)
    _lib.check(lib.vsr_conv3x3_c64_fwd(dtype, _ptr(x_pm), _ptr(_f32c(weight)), _ptr(None if bias is None else _f32c(bias)),
                                       _ptr(wpack), _ptr(y), _ptr(res_pm), act, n, h, w, _stream()), "conv3x3_c64_fwd")
    return y


def chain_timeouts() -> int:
    """Dependency waits the trunk-chain kernel (csrc/conv3x3_chain.hip) has given up since the library was loaded (1 s each).
    Anything but 0 means some launch ran on unfinished inputs.  Such a launch poisons its own output with NaN on the device
    (chain_poison_kernel: sr, the loss and the gradient norm go non-finite, FusedAdam skips the step), so the counter is for
    diagnosis.  Synchronises the device."""
    import ctypes
    out = ctypes.c_uint(0)
    _lib.check(_lib.load().vsr_debug_chain_timeouts(ctypes.byref(out)), "debug_chain_timeouts")
    return int(out.value)


_chain_timeouts_seen = 0


def raise_on_chain_timeout(where: str = "") -> None:
    """For the places of a training loop that synchronise anyway (reading the loss, a checkpoint, `rewind_skipped_step`):
    raise if a chain launch has given up a dependency wait since the last call.  The launch concerned has already turned its
    outputs into NaN; this names the cause (a long foreign kernel, a debugger or another process holding the GPU's CUs)."""
    global _chain_timeouts_seen
    n = chain_timeouts()
    if n != _chain_timeouts_seen:
        new, _chain_timeouts_seen = n - _chain_timeouts_seen, n
        raise RuntimeError(f"vsrlab_amd: {new} dependency wait(s) of the trunk-chain kernel timed out{' (' + where + ')' if where else ''}: "
                           "the affected launches wrote NaN into their outputs; VSRLAB_AMD_CHAIN=0 runs one launch per layer")


class ResidualChainC64:
    """The body of ResidualBlock.res_block (conv.py:85-92, 99-103) as ONE launch (vsr_conv3x3_c64_chain_fwd): `blocks`
    ResidualConv blocks on a blocked 64-channel bf16 image, every intermediate kept.  Holds one allocation with the
    2*blocks + 1 images, the packed weights, the biases and the launch's flag words; call it with x_pm to run the chain,
    `image(l)` is layer l's input (image(2*blocks) = the output)."""

    def __init__(self, weights, biases, n: int, h: int, w: int, device):
        assert len(weights) == len(biases) and len(weights) >= 1
        lib = _lib.load()
        self.L, self.n, self.h, self.w = len(weights), n, h, w
        self.img_elems = n * h * ((w + 31) // 32) * 32 * 64
        al = lambda b: (b + 255) // 256 * 256
        o_w = al((self.L + 1) * self.img_elems * 2)
        o_b = o_w + al(self.L * 9 * 64 * 64 * 2)
        o_s = o_b + al(self.L * 64 * 4)
        nsync = lib.vsr_conv3x3_c64_chain_sync_bytes(self.L, n, h, w)
        if nsync == 0:
            raise ValueError("vsrlab_amd: unsupported chain shape")
        self.buf = torch.zeros(o_s + nsync + 512, dtype=torch.uint8, device=device)
        pad = (-self.buf.data_ptr()) % 256
        self.buf = self.buf[pad:]
        self.images = self.buf[:(self.L + 1) * self.img_elems * 2].view(torch.bfloat16)
        self.wpack = self.buf[o_w:o_w + self.L * 9 * 64 * 64 * 2].view(torch.bfloat16)
        self.bias = self.buf[o_b:o_b + self.L * 64 * 4].view(torch.float32)
        self.sync = self.buf[o_s:o_s + nsync]
        scratch = torch.empty(self.img_elems, dtype=torch.bfloat16, device=device)
        for l, (wt, b) in enumerate(zip(weights, biases)):          # vsr_conv3x3_c64_fwd packs a weight set as a side effect
            _lib.check(lib.vsr_conv3x3_c64_fwd(DT_BF16, _ptr(self.image(0)), _ptr(_f32c(wt)), _ptr(None), _ptr(self.wpack[l * 9 * 64 * 64:]),
                                               _ptr(scratch), _ptr(None), 0, n, h, w, _stream()), "conv3x3_c64_fwd")
            self.bias[l * 64:(l + 1) * 64] = 0.0 if b is None else _f32c(b)

    def image(self, l: int) -> torch.Tensor:
        return self.images[l * self.img_elems:(l + 1) * self.img_elems]

    def launch(self):
        lib = _lib.load()
        _lib.check(lib.vsr_conv3x3_c64_chain_fwd(_ptr(self.images), _ptr(self.wpack), _ptr(self.bias), self.L, self.n, self.h, self.w,
                                                 _ptr(self.sync), _stream()), "conv3x3_c64_chain_fwd")

    def __call__(self, x_pm: torch.Tensor) -> torch.Tensor:
        _require_gpu(x_pm)
        assert x_pm.dtype == torch.bfloat16 and x_pm.numel() == self.img_elems
        self.image(0).copy_(x_pm.reshape(-1))
        self.launch()
        return self.image(self.L)


def conv3x3_c64_dgrad(dy_pm: torch.Tensor, weight: torch.Tensor, res_pm: Optional[torch.Tensor] = None,
                      aux_pm: Optional[torch.Tensor] = None, mask_mode: int = 0) -> torch.Tensor:
    _require_gpu(dy_pm, weight)
    n, h, w, c = _pm_dims(dy_pm)
    dtype = DT_BF16 if dy_pm.dtype == torch.bfloat16 else DT_F32
    lib = _lib.load()
    wpack = torch.empty(9 * 64 * 64, dtype=dy_pm.dtype, device=dy_pm.device)
    dx = _pm_like(dy_pm)
    _lib.check(lib.vsr_conv3x3_c64_dgrad(dtype, _ptr(dy_pm), _ptr(_f32c(weight)), _ptr(wpack), _ptr(dx), _ptr(res_pm),
                                         _ptr(aux_pm), mask_mode, n, h, w, _stream()), "conv3x3_c64_dgrad")
    return dx


def conv3x3_c64_wgrad(x_pm: torch.Tensor, dy_pm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _require_gpu(x_pm, dy_pm)
    n, h, w, c = _pm_dims(x_pm)
    dtype = DT_BF16 if x_pm.dtype == torch.bfloat16 else DT_F32
    lib = _lib.load()
    slab = torch.empty(lib.vsr_conv3x3_c64_wgrad_slab_floats(), dtype=torch.float32, device=x_pm.device)
    gw = torch.empty((64, 64, 3, 3), dtype=torch.float32, device=x_pm.device)
    gb = torch.empty((64,), dtype=torch.float32, device=x_pm.device)
    _lib.check(lib.vsr_conv3x3_c64_wgrad(dtype, _ptr(x_pm), _ptr(dy_pm), _ptr(gw), _ptr(gb), _ptr(slab), n, h, w, _stream()),
               "conv3x3_c64_wgrad")
    return gw, gb


class _ResidualConvFn(torch.autograd.Function):
    """x + conv2(relu(conv1(x))) with its full backward, channels = 64 (conv.py:89-92)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dtype):
        xp = to_pixel_major(x, dtype)
        a = conv3x3_c64(xp, w1, b1, act=1)
        y = conv3x3_c64(a, w2, b2, act=0, res_pm=xp)
        ctx.save_for_backward(xp, a, w1, w2)
        return from_pixel_major(y)

    @staticmethod
    def backward(ctx, gy):
        xp, a, w1, w2 = ctx.saved_tensors
        dtype = DT_BF16 if xp.dtype == torch.bfloat16 else DT_F32
        g = to_pixel_major(gy, dtype)
        ga = conv3x3_c64_dgrad(g, w2, aux_pm=a, mask_mode=1)
        gx = conv3x3_c64_dgrad(ga, w1, res_pm=g)
        gw2, gb2 = conv3x3_c64_wgrad(a, g)
        gw1, gb1 = conv3x3_c64_wgrad(xp, ga)
        return from_pixel_major(gx), gw1, gb1, gw2, gb2, None


def residual_conv(x, w1, b1, w2, b2, compute_dtype: Optional[str] = None):
    _require_gpu(x)
    c = x.shape[1]
    _check_width(c, "ResidualConv")
    if c == 64:
        return _ResidualConvFn.apply(x, w1, b1, w2, b2, resolve_dtype(compute_dtype))
    # 16 / 32 channels: the two convs as vsr_conv_layer_fwd / _bwd layers, the identity added by autograd
    a = _conv_layer_autograd(x, None, w1, b1, 1, compute_dtype=compute_dtype)
    return x + _conv_layer_autograd(a, None, w2, b2, 0, compute_dtype=compute_dtype)


# --------------------------------------------------------------------------------------------- #
# single conv layers of the reference's building blocks (ConvReLU, the ResidualBlock stem, PixelShufflePack, SpynetModule's
# layers): forward vsr_conv_layer_fwd, backward vsr_conv_layer_bwd -- ordinary autograd modules, like the reference's
# --------------------------------------------------------------------------------------------- #
def conv_layer(x_pm: Optional[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0, slope: float = 0.1,
               lr_planar: Optional[torch.Tensor] = None, pixel_shuffle: bool = False, planar_out: bool = False,
               dtype: Optional[int] = None, hw: Optional[Tuple[int, int, int]] = None) -> torch.Tensor:
    """``vsr_conv_layer_fwd``: one conv layer on a blocked pixel-major tensor (or the planar LR frames).  Returns a
    pixel-major tensor, or (N,cout,H,W) fp32 when ``planar_out``."""
    lib = _lib.load()
    cout, cin, ks, _ = weight.shape
    if x_pm is not None:
        n, h, w, cin_pm = _pm_dims(x_pm)
        dt = DT_BF16 if x_pm.dtype == torch.bfloat16 else DT_F32
        dev = x_pm.device
    else:
        n, h, w = hw
        cin_pm, dt, dev = 0, dtype, lr_planar.device
    wpack = torch.empty(49 * 64 * 64 * 4, dtype=_TORCH_DT[dt], device=dev)
    y_pm = y_pl = None
    cd = 0
    if planar_out:
        y_pl = torch.empty((n, cout, h, w), dtype=torch.float32, device=dev)
    else:
        cd = cout // 4 if pixel_shuffle else max(16, cout)
        s = 2 if pixel_shuffle else 1
        y_pm = torch.empty((n, s * h, (s * w + 31) // 32, cd // 8, 32, 8), dtype=_TORCH_DT[dt], device=dev)
        y_pm.pm_w = s * w
    _lib.check(lib.vsr_conv_layer_fwd(dt, ks, _ptr(x_pm), cin_pm, _ptr(None if lr_planar is None else _f32c(lr_planar)), _ptr(_f32c(weight)),
                                      _ptr(None if bias is None else _f32c(bias)), cin, cout, _ptr(wpack), _ptr(y_pm), cd, _ptr(y_pl),
                                      act, float(slope), int(pixel_shuffle), n, h, w, _stream()), "conv_layer_fwd")
    return y_pl if planar_out else y_pm


class _ConvLayerFn(torch.autograd.Function):
    """y = act(conv(x [, lr]) + b) [+ PixelShuffle(2)] on planar (N,C,H,W) tensors; x / lr may be None (stems).  Backward =
    ``vsr_conv_layer_bwd``: data gradient(s), weight gradient, bias gradient."""

    @staticmethod
    def forward(ctx, x, lr, weight, bias, act, slope, pixel_shuffle, planar_out, dt):
        cout, cin = weight.shape[:2]
        ref = x if x is not None else lr
        n, _, h, w = ref.shape
        x_pm = None
        if x is not None:
            x_pm = to_pixel_major(x, dt, ((x.shape[1] + 15) // 16) * 16)
        lr32 = None if lr is None else _f32c(lr)
        y = conv_layer(x_pm, weight, bias, act=act, slope=slope, lr_planar=lr32, pixel_shuffle=pixel_shuffle, planar_out=planar_out,
                       dtype=dt, hw=(n, h, w))
        ctx.save_for_backward(x_pm, lr32, weight, y)
        ctx.meta = (act, float(slope), bool(pixel_shuffle), bool(planar_out), dt, n, h, w, cin, cout, None if x is None else x.shape[1],
                    x_pm.pm_w if x_pm is not None else None, bias is not None)
        if planar_out:
            return y
        return from_pixel_major(y, cout // 4 if pixel_shuffle else cout)

    @staticmethod
    def backward(ctx, dout):
        x_pm, lr32, weight, y = ctx.saved_tensors
        act, slope, ps, planar, dt, n, h, w, cin, cout, xc, xw, has_bias = ctx.meta
        lib = _lib.load()
        dev = dout.device
        if x_pm is not None:
            x_pm.pm_w = xw
        need_x, need_lr, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        cd = 0 if planar else (cout // 4 if ps else max(16, cout))
        dy_pm = dy_pl = y_pm = y_pl = None
        if planar:
            dy_pl, y_pl = _f32c(dout), y
        else:
            dy_pm = to_pixel_major(dout, dt, cd)
            y_pm = y
        dx_pm = None
        if need_x and x_pm is not None:
            dx_pm = torch.empty_like(x_pm)
            dx_pm.pm_w = xw
        dlr = torch.empty_like(lr32) if (need_lr and lr32 is not None) else None
        gw = torch.empty(weight.shape, dtype=torch.float32, device=dev) if (need_w or need_b) else None
        gb = torch.empty(cout, dtype=torch.float32, device=dev) if (need_b and has_bias) else None
        nbytes = lib.vsr_conv_layer_bwd_scratch_bytes(dt, n, h, w, int(ps))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ks = weight.shape[2]
        _lib.check(lib.vsr_conv_layer_bwd(dt, ks, _ptr(x_pm), 0 if x_pm is None else x_pm.shape[3] * 8, _ptr(lr32), _ptr(_f32c(weight)), cin, cout,
                                          _ptr(y_pm), _ptr(y_pl), _ptr(dy_pm), _ptr(dy_pl), cd, act, slope, int(ps), _ptr(dx_pm), _ptr(dlr),
                                          _ptr(gw), _ptr(gb), _ptr(scratch), nbytes, n, h, w, _stream()), "conv_layer_bwd")
        dx = from_pixel_major(dx_pm, xc) if dx_pm is not None else None
        return dx, dlr, (gw if need_w else None), gb, None, None, None, None, None


def _conv_layer_autograd(x, lr, weight, bias, act, slope=0.1, pixel_shuffle=False, planar_out=False, compute_dtype=None):
    return _ConvLayerFn.apply(x, lr, weight, bias, act, slope, pixel_shuffle, planar_out, resolve_dtype(compute_dtype))


def conv_relu_forward(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], compute_dtype: Optional[str] = None) -> torch.Tensor:
    """ConvReLU.forward (core/modules/conv.py:15-22) for the SPyNet layer shapes (7x7) and 64 -> 64 (3x3 / 1x1); differentiable."""
    _require_gpu(x)
    cout = weight.shape[0]
    return _conv_layer_autograd(x, None, weight, bias, 1, planar_out=cout <= 4, compute_dtype=compute_dtype)


def pixel_shuffle_pack_forward(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], compute_dtype: Optional[str] = None):
    """PixelShufflePack.forward (upsampling.py:10-12): conv3x3 C -> 4C + PixelShuffle(2), C = 16, 32 or 64; the shuffle is the
    store pattern; differentiable."""
    _require_gpu(x)
    c = x.shape[1]
    if c not in MID_CHANNELS or tuple(weight.shape) != (4 * c, c, 3, 3):
        raise NotImplementedError("the HIP PixelShufflePack is built for C -> C channels, scale 2 (the reference's use), C = 16, 32 or 64")
    return _conv_layer_autograd(x, None, weight, bias, 0, pixel_shuffle=True, compute_dtype=compute_dtype)


def residual_block_forward(x: torch.Tensor, stem_w: torch.Tensor, stem_b: torch.Tensor, blocks: Sequence[Tuple[torch.Tensor, ...]],
                           compute_dtype: Optional[str] = None) -> torch.Tensor:
    """ResidualBlock.forward (core/modules/conv.py:94-103) on x = cat([lr(3), feat(64)]) (the trunks) or x = lr (the pre-clean
    stack): conv3x3 + LeakyReLU(0.1), then the ResidualConv blocks ((w1, b1, w2, b2) each); differentiable (the stem through
    vsr_conv_layer_bwd, the blocks through the ResidualConv function)."""
    _require_gpu(x)
    n, cin, h, w = x.shape
    mid = stem_w.shape[0]
    if mid not in MID_CHANNELS:
        raise NotImplementedError(f"the HIP ResidualBlock is built for mid_channels 16, 32 or 64, not {mid}")
    if cin == 3 + mid:
        y = _conv_layer_autograd(x[:, 3:].contiguous(), x[:, :3].contiguous(), stem_w, stem_b, 2, compute_dtype=compute_dtype)
    elif cin == 3:
        y = _conv_layer_autograd(None, x, stem_w, stem_b, 2, compute_dtype=compute_dtype)
    else:
        raise NotImplementedError(f"the HIP ResidualBlock stem takes 3 (pre-clean) or 3 + {mid} (trunk) input channels")
    for (w1, b1, w2, b2) in blocks:
        y = residual_conv(y, w1, b1, w2, b2, compute_dtype)
    return y
