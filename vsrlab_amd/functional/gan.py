"""The losses of RealBasicVSR's GAN stage: Charbonnier, fused value + gradient (reference: core/losses.py:10-18;
csrc/layer_ops.hip), the discriminator with spectral norm and BCE (csrc/disc_engine.hip, csrc/conv_wide.hip) and the VGG19
perceptual loss (core/losses.py:8,29-64; csrc/perceptual_engine.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from .. import _lib
from .._lib import DT_F32
from ._base import _backward_once, _f32c, _ptr, _ptr_array, _require_gpu, _stream, resolve_dtype
from .conv import _conv_layer_autograd


class _CharbonnierFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, eps):
        lib = _lib.load()
        x32, y32 = _f32c(x), _f32c(y)
        dx = torch.empty_like(x32)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        scratch = torch.empty(lib.vsr_charbonnier_scratch_floats(), dtype=torch.float32, device=x.device)
        _lib.check(lib.vsr_charbonnier_fwd_bwd(_ptr(x32), _ptr(y32), _ptr(dx), _ptr(loss), _ptr(scratch), x32.numel(), float(eps), _stream()),
                   "charbonnier")
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None, None


def charbonnier_loss(x: torch.Tensor, y: torch.Tensor, eps: float = 1e-9) -> torch.Tensor:
    _require_gpu(x, y)
    if y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("HIP Charbonnier differentiates w.r.t. its first argument only")
    return _CharbonnierFn.apply(x, y, eps)


# --------------------------------------------------------------------------------------------- #
# GAN side (BASELINE config 3): UNetDiscriminator + spectral norm + BCE-with-logits
# (reference: vsr/models/RealBasicVSR/modules/unet-discriminator.py:4-31, core/modules/conv.py:6-13,
#  core/losses.py:66-74)
# --------------------------------------------------------------------------------------------- #
_DISC_SPECTRAL = [(128, 64, 4), (256, 128, 4), (512, 256, 4), (256, 512, 3), (128, 256, 3), (64, 128, 3), (64, 64, 3), (64, 64, 3)]


class _DiscriminatorFn(torch.autograd.Function):
    """logits = UNetDiscriminator(img).  Inputs: img, then conv_0.weight, conv_0.bias, the 8 weight_orig tensors,
    conv_9.weight, conv_9.bias (autograd leaves), then the 8 (u, v) buffer pairs (updated IN PLACE by the training-mode
    power iteration, like torch.nn.utils.spectral_norm's forward pre-hook)."""

    @staticmethod
    def forward(ctx, img, dtype, training, need_bwd, *tensors):
        from .._lib import DiscDesc
        lib = _lib.load()
        n, c, h, w = img.shape
        params, bufs = tensors[:12], tensors[12:]
        dev = img.device
        img32 = _f32c(img)
        p32 = [_f32c(p) for p in params]
        eff, sig, uv = [], [], []
        for k, (co, ci, ks) in enumerate(_DISC_SPECTRAL):
            worig = p32[2 + k]
            u, v = bufs[2 * k], bufs[2 * k + 1]
            weff = torch.empty_like(worig)
            sigma = torch.empty(1, dtype=torch.float32, device=dev)
            _lib.check(lib.vsr_spectral_norm(_ptr(worig), _ptr(u), _ptr(v), _ptr(weff), _ptr(sigma), co, ci * ks * ks, int(training),
                                             _stream()), "spectral_norm")
            eff.append(weff)
            sig.append(sigma)
            uv.append((u.detach().clone(), v.detach().clone()) if need_bwd else None)   # the constants of THIS forward's graph
        desc = DiscDesc(n, h, w, 64, dtype)
        nbytes = lib.vsr_disc_workspace_bytes(ctypes.byref(desc), int(need_bwd))
        if nbytes == 0:
            raise RuntimeError(f"vsrlab_amd: unsupported discriminator input for the HIP path: {(n, c, h, w)} "
                               "(3-channel frames, height and width multiples of 8, mid_ch = 64)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call = [p32[0], p32[1]] + eff + [p32[10], p32[11]]
        out = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
        _lib.check(lib.vsr_disc_forward(ctypes.byref(desc), _ptr_array(call), 12, _ptr(img32), _ptr(out), _ptr(ws), ws.numel(),
                                        int(need_bwd), _stream()), "disc_forward")
        ctx.need_bwd = need_bwd
        if need_bwd:
            ctx.ws, ctx.img32, ctx.p32, ctx.sig, ctx.uv, ctx.desc_args = ws, img32, p32, sig, uv, (n, h, w, 64, dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .._lib import DiscDesc
        if not ctx.need_bwd:
            raise RuntimeError("vsrlab_amd: backward through a discriminator forward that ran without need_backward")
        if ctx.ws is None:
            raise RuntimeError("vsrlab_amd: trying to backward through the discriminator graph a second time")
        lib = _lib.load()
        desc = DiscDesc(*ctx.desc_args)
        p32 = ctx.p32
        need_p = [bool(ctx.needs_input_grad[4 + k]) for k in range(12)]
        any_p = any(need_p)
        geff = [torch.zeros_like(p) if any_p else None for p in p32]
        dimg = torch.empty_like(ctx.img32) if ctx.needs_input_grad[0] else None
        _lib.check(lib.vsr_disc_backward(ctypes.byref(desc), _ptr_array(geff), 12, _ptr(ctx.img32), _ptr(_f32c(dout)), _ptr(dimg),
                                         _ptr(ctx.ws), ctx.ws.numel(), _stream()), "disc_backward")
        grads = [None] * 12
        if any_p:
            grads[0], grads[1], grads[10], grads[11] = geff[0], geff[1], geff[10], geff[11]
            sn_scratch = torch.empty(1024, dtype=torch.float32, device=dout.device)      # VSR_SN_SCRATCH_FLOATS
            for k, (co, ci, ks) in enumerate(_DISC_SPECTRAL):
                gorig = torch.zeros_like(p32[2 + k])
                u, v = ctx.uv[k]
                _lib.check(lib.vsr_spectral_norm_backward(_ptr(geff[2 + k]), _ptr(p32[2 + k]), _ptr(u), _ptr(v), _ptr(ctx.sig[k]),
                                                          _ptr(gorig), co, ci * ks * ks, _ptr(sn_scratch), _stream()), "spectral_norm_backward")
                grads[2 + k] = gorig
        ctx.ws = None
        return (dimg, None, None, None) + tuple(g if need_p[k] else None for k, g in enumerate(grads)) + (None,) * 16


class _SpectralNormFn(torch.autograd.Function):
    """weight = weight_orig / sigma(weight_orig; u, v): torch.nn.utils.spectral_norm's ``compute_weight`` (one power iteration per
    training-mode forward, u and v updated IN PLACE, sigma = u . (W v) differentiated through W only) as ``vsr_spectral_norm`` /
    ``vsr_spectral_norm_backward`` -- what the discriminator function above does for its eight inner layers, for ONE layer."""

    @staticmethod
    def forward(ctx, worig, u, v, training):
        lib = _lib.load()
        w32 = _f32c(worig)
        co = w32.shape[0]
        k = w32.numel() // co
        weff = torch.empty_like(w32)
        sigma = torch.empty(1, dtype=torch.float32, device=w32.device)
        _lib.check(lib.vsr_spectral_norm(_ptr(w32), _ptr(u), _ptr(v), _ptr(weff), _ptr(sigma), co, k, int(training), _stream()), "spectral_norm")
        ctx.save_for_backward(w32, u.detach().clone(), v.detach().clone(), sigma)          # the constants of THIS forward's graph
        return weff

    @staticmethod
    def backward(ctx, geff):
        w32, u, v, sigma = ctx.saved_tensors
        lib = _lib.load()
        co = w32.shape[0]
        gorig = torch.zeros_like(w32)
        scratch = torch.empty(1024, dtype=torch.float32, device=w32.device)                 # VSR_SN_SCRATCH_FLOATS
        _lib.check(lib.vsr_spectral_norm_backward(_ptr(_f32c(geff)), _ptr(w32), _ptr(u), _ptr(v), _ptr(sigma), _ptr(gorig), co, w32.numel() // co,
                                                  _ptr(scratch), _stream()), "spectral_norm_backward")
        return gorig, None, None, None


def spectral_conv_forward(x: torch.Tensor, weight_orig: torch.Tensor, u: torch.Tensor, v: torch.Tensor, training: bool,
                          compute_dtype: Optional[str] = None) -> torch.Tensor:
    """SpectralConv.forward (core/modules/conv.py:6-13) on its own, for the shape the per-layer kernels serve: 3x3, stride 1,
    padding 1, 64 -> 64 (the discriminator's conv_7 / conv_8 shape; the wide and the 4x4 stride-2 layers exist only inside the
    discriminator engine).  Differentiable w.r.t. x and weight_orig; u / v are updated in place when ``training``."""
    _require_gpu(x, weight_orig)
    if tuple(weight_orig.shape) != (64, 64, 3, 3) or x.shape[1] != 64:
        raise NotImplementedError("standalone HIP SpectralConv: Conv2d(64, 64, 3, 1, 1); other shapes run inside UNetDiscriminator")
    weff = _SpectralNormFn.apply(weight_orig, u, v, bool(training))
    return _conv_layer_autograd(x, None, weff, None, 0, compute_dtype=compute_dtype)


def discriminator_forward(img: torch.Tensor, params: Sequence[torch.Tensor], buffers: Sequence[torch.Tensor], training: bool,
                          compute_dtype: Optional[str] = None) -> torch.Tensor:
    """``params``: conv_0.weight, conv_0.bias, conv_1..8 ``weight_orig``, conv_9.weight, conv_9.bias; ``buffers``:
    (weight_u, weight_v) of conv_1..8, updated in place when ``training``."""
    _require_gpu(img)
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("discriminator input must be (N,3,H,W)")
    if len(params) != 12 or len(buffers) != 16:
        raise ValueError("expected 12 parameter tensors and 16 spectral-norm buffers")
    need_bwd = torch.is_grad_enabled() and (img.requires_grad or any(p.requires_grad for p in params))
    return _DiscriminatorFn.apply(img, resolve_dtype(compute_dtype), bool(training), need_bwd, *params, *buffers)


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        lib = _lib.load()
        x32 = _f32c(x)
        dx = torch.empty_like(x32)
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        _lib.check(lib.vsr_bce_with_logits(_ptr(x32), float(target), _ptr(dx), _ptr(loss), x32.numel(), _stream()), "bce_with_logits")
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None


def bce_with_logits_const(x: torch.Tensor, target: float) -> torch.Tensor:
    """mean BCE-with-logits of ``x`` against the constant ``target`` (AdversarialLoss, core/losses.py:70-73)."""
    _require_gpu(x)
    return _BCEFn.apply(x, float(target))


# --------------------------------------------------------------------------------------------- #
# VGG19 perceptual loss (reference: core/losses.py:8,29-64)
# --------------------------------------------------------------------------------------------- #
PERCEPTUAL_LAYER_WEIGHTS = {'2': 0.1, '7': 0.1, '16': 0.8, '25': 0.9, '34': 1.0}
# (features index, cout, cin) of the 16 convolutions of vgg19().features[:35]
VGG19_CONVS = ((0, 64, 3), (2, 64, 64), (5, 128, 64), (7, 128, 128), (10, 256, 128), (12, 256, 256), (14, 256, 256), (16, 256, 256),
               (19, 512, 256), (21, 512, 512), (23, 512, 512), (25, 512, 512), (28, 512, 512), (30, 512, 512), (32, 512, 512),
               (34, 512, 512))
_TAP_CHANNELS = (64, 128, 256, 512, 512)
_TAP_LEVELS = (0, 1, 2, 3, 4)
DEFAULT_PERCEPTUAL_WORKSPACE = 16 << 30


def _perceptual_desc(n: int, h: int, w: int, dtype: int, need_grad: bool):
    from .._lib import PerceptualDesc
    return PerceptualDesc(int(n), int(h), int(w), int(dtype), int(bool(need_grad)))


def perceptual_workspace_bytes(n: int, h: int, w: int, dtype: int = DT_F32, need_grad: bool = True) -> int:
    """Device workspace of one ``vsr_perceptual_loss`` call on ``n`` images of h x w (0: unsupported).  Host arithmetic only."""
    return int(_lib.load().vsr_perceptual_workspace_bytes(ctypes.byref(_perceptual_desc(n, h, w, dtype, need_grad))))


def perceptual_chunk(n: int, h: int, w: int, dtype: int, need_grad: bool, max_workspace_bytes: Optional[int] = None) -> int:
    """Images per call such that the workspace stays within the budget (at least 1: one image is the unit of work)."""
    budget = DEFAULT_PERCEPTUAL_WORKSPACE if max_workspace_bytes is None else int(max_workspace_bytes)
    one = perceptual_workspace_bytes(1, h, w, dtype, need_grad)
    per = perceptual_workspace_bytes(2, h, w, dtype, need_grad) - one
    if one == 0 or one > budget:
        return 1
    return int(max(1, min(n, 1 + (budget - one) // max(per, 1))))


def _tap_numels(n: int, h: int, w: int):
    out = []
    for c, lv in zip(_TAP_CHANNELS, _TAP_LEVELS):
        hh, ww = h, w
        for _ in range(lv):
            hh, ww = hh // 2, ww // 2
        out.append(n * c * hh * ww)
    return out


class _PerceptualFn(torch.autograd.Function):
    """loss = weight * sum_k LAYER_WEIGHTS[k] * mean|f_k(sr) - f_k(hr)|.  d loss / d sr is computed during the forward (one
    engine call per chunk of images) and is all the backward keeps; hr gets no gradient."""

    @staticmethod
    def forward(ctx, sr, hr, dtype, weight, chunk, need_grad, terms_out, *params):
        lib = _lib.load()
        h, w = hr.shape[-2], hr.shape[-1]
        sr4, hr4 = _f32c(sr).reshape(-1, 3, h, w), _f32c(hr).reshape(-1, 3, h, w)
        n = sr4.shape[0]
        p32 = [_f32c(p) for p in params]
        lw = list(PERCEPTUAL_LAYER_WEIGHTS.values())
        numels = _tap_numels(n, h, w)
        scales = (ctypes.c_float * 5)(*[float(weight) * lw[k] / numels[k] for k in range(5)])
        dev = sr4.device
        sums = torch.empty((n, 5), dtype=torch.float64, device=dev)
        dsr = torch.empty_like(sr4) if need_grad else None
        nbytes = perceptual_workspace_bytes(min(chunk, n), h, w, dtype, need_grad)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        parr = _ptr_array(p32)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            desc = _perceptual_desc(m, h, w, dtype, need_grad)
            _lib.check(lib.vsr_perceptual_loss(ctypes.byref(desc), parr, 32, _ptr(sr4[i:i + m]), _ptr(hr4[i:i + m]),
                                               scales if need_grad else None, _ptr(sums[i:i + m]),
                                               _ptr(dsr[i:i + m] if need_grad else None), _ptr(ws), nbytes, _stream()), "perceptual_loss")
        del ws
        coef = torch.tensor([float(weight) * lw[k] / numels[k] for k in range(5)], dtype=torch.float64, device=dev)
        terms = sums.sum(0) * coef
        if terms_out is not None:
            terms_out.append(terms)
        ctx.dsr = dsr.reshape(sr.shape) if need_grad else None
        ctx.backward_done = False
        ctx.sr_dtype = sr.dtype
        return terms.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        _backward_once(ctx, "perceptual_loss", ctx.dsr is not None, noun="perceptual loss")
        dsr, ctx.dsr, ctx.backward_done = ctx.dsr, None, True
        return (g * dsr).to(ctx.sr_dtype), None, None, None, None, None, None, *([None] * 32)


def perceptual_loss(sr: torch.Tensor, hr: torch.Tensor, params: Sequence[torch.Tensor], weight: float = 1.0,
                    compute_dtype: Optional[str] = None, max_workspace_bytes: Optional[int] = None,
                    return_terms: bool = False):
    """PerceptualLoss.forward (core/losses.py:47-64) on the HIP path.  ``sr``, ``hr``: (..., 3, h, w), h, w >= 16.  ``params``: the
    32 tensors of vgg19().features[:35] (weight, bias of features.{0,2,5,...,34}).  The batch runs in chunks whose workspace
    stays within ``max_workspace_bytes`` (default 16 GiB).  ``return_terms``: also return the five weighted tap terms (fp64)."""
    if sr.shape != hr.shape or sr.dim() < 3 or sr.shape[-3] != 3:
        raise ValueError(f"perceptual_loss: sr and hr must have one shape (..., 3, h, w); got {tuple(sr.shape)} and {tuple(hr.shape)}")
    h, w = hr.shape[-2], hr.shape[-1]
    if h < 16 or w < 16 or sr.numel() == 0:
        raise ValueError(f"perceptual_loss: frames must be at least 16 x 16 (four 2x2 max-pools), got {h} x {w}")
    if len(params) != 32:
        raise ValueError(f"perceptual_loss: expected the 32 weight / bias tensors of vgg19().features[:35], got {len(params)}")
    for (idx, co, ci), wt, b in zip(VGG19_CONVS, params[0::2], params[1::2]):
        if tuple(wt.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
            raise ValueError(f"perceptual_loss: features.{idx} must be Conv2d({ci}, {co}, 3): got {tuple(wt.shape)} / {tuple(b.shape)}")
    _require_gpu(sr, hr, *params)
    dtype = resolve_dtype(compute_dtype)
    n = sr.numel() // (3 * h * w)
    need_grad = torch.is_grad_enabled() and sr.requires_grad
    chunk = perceptual_chunk(n, h, w, dtype, need_grad, max_workspace_bytes)
    terms = [] if return_terms else None
    loss = _PerceptualFn.apply(sr, hr.detach(), dtype, float(weight), chunk, need_grad, terms, *params)
    return (loss, terms[0]) if return_terms else loss
