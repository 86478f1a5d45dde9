"""RAFT's correlation lookup without the all-pairs volume (reference: optical_flow/models/raft/corr.py; csrc/raft_corr.hip),
then the local correlation (csrc/spatial_corr.hip, built into libvsrlab_spatial_corr.so)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _lib
from .._lib import DT_F32
from ._base import _backward_once, _f32c, _pair, _ptr, _require_gpu, _stream, resolve_dtype


_RAFT_UNSUPPORTED = ("vsrlab_amd: raft_corr: unsupported shape (D = 128, radius 3, 1..4 levels, every pooled level at least "
                     "2 x 2): fmap {shape}, num_levels {levels}, radius {radius}")


def raft_corr_workspace_bytes(fmap_shape, num_levels: int = 4, radius: int = 3, dtype: int = DT_F32, gradients: bool = False) -> int:
    """Bytes of the packed maps of one pyramid (``gradients=False``) or of its fp32 gradient accumulators; 0: unsupported
    shape.  Host arithmetic only."""
    n, d, h, w = fmap_shape
    desc = _lib.RaftCorrDesc(int(n), int(d), int(h), int(w), int(num_levels), int(radius), int(dtype))
    return int(_lib.load().vsr_raft_corr_workspace_bytes(ctypes.byref(desc), int(bool(gradients))))


class _RaftCorrState:
    """Device state of one pyramid, shared by the autograd nodes of the pyramid and of its lookups (it does not refer to them:
    no reference cycle through the graph)."""

    def __init__(self, desc, packed, shape, num_levels, need_bwd):
        self.desc, self.packed, self.shape, self.num_levels, self.need_bwd = desc, packed, tuple(shape), num_levels, need_bwd
        self.gacc = None                        # fp32 gradient accumulators, allocated by the first lookup backward


class RaftCorrPyramid:
    """What ``raft_corr_pyramid`` returns: the packed fmap1 and the pooled levels of fmap2 on the device, for any number of
    ``raft_corr_lookup`` calls.  The gradients of all those lookups are summed in fp32 accumulators and leave through the
    pyramid's own backward, once (``token`` is what ties the lookups to it in the autograd graph)."""

    def __init__(self, state, token):
        self.state, self.token = state, token
        self.shape, self.num_levels = state.shape, state.num_levels

    @property
    def out_channels(self):
        return self.num_levels * 49

    @property
    def packed_bytes(self):
        return self.state.packed.numel()


class _RaftPyramidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap1, fmap2, handle):
        f1, f2 = _f32c(fmap1), _f32c(fmap2)
        _lib.check(_lib.load().vsr_raft_corr_pyramid_fwd(ctypes.byref(handle.desc), _ptr(f1), _ptr(f2), _ptr(handle.packed),
                                                         handle.packed.numel(), _stream()), "raft_corr_pyramid_fwd")
        ctx.handle = handle
        ctx.dtypes = (fmap1.dtype, fmap2.dtype)
        ctx.backward_done = False
        return torch.zeros(1, dtype=torch.float32, device=f1.device)

    @staticmethod
    def backward(ctx, gtoken):
        _backward_once(ctx, "raft_corr_pyramid")
        ctx.backward_done = True
        h = ctx.handle
        gacc, h.gacc = h.gacc, None
        if gacc is None:                        # no lookup of this pyramid was differentiated
            return None, None, None
        need = ctx.needs_input_grad
        dev = gacc.device
        d1 = torch.empty(h.shape, dtype=torch.float32, device=dev) if need[0] else None
        d2 = torch.empty(h.shape, dtype=torch.float32, device=dev) if need[1] else None
        _lib.check(_lib.load().vsr_raft_corr_pyramid_bwd(ctypes.byref(h.desc), _ptr(gacc), gacc.numel(), _ptr(d1), _ptr(d2), _stream()),
                   "raft_corr_pyramid_bwd")
        del gacc
        return (None if d1 is None else d1.to(ctx.dtypes[0]), None if d2 is None else d2.to(ctx.dtypes[1]), None)


class _RaftLookupFn(torch.autograd.Function):
    """out = the 7 x 7 windows of every level at ``coords``.  The backward adds into the pyramid's accumulators: d fmap1 is
    bit-identical across runs, d fmap2 is summed with fp32 atomic adds (reproducible to rounding).  ``coords`` gets no gradient."""

    @staticmethod
    def forward(ctx, token, coords, handle):
        n, _, h, w = handle.shape
        c32 = _f32c(coords)
        out = torch.empty((n, handle.num_levels * 49, h, w), dtype=torch.float32, device=c32.device)
        _lib.check(_lib.load().vsr_raft_corr_lookup_fwd(ctypes.byref(handle.desc), _ptr(handle.packed), handle.packed.numel(), _ptr(c32),
                                                        _ptr(out), _stream()), "raft_corr_lookup_fwd")
        ctx.handle = handle
        ctx.coords = c32 if handle.need_bwd else None
        ctx.backward_done = False
        return out

    @staticmethod
    def backward(ctx, gout):
        _backward_once(ctx, "raft_corr_lookup", ctx.coords is not None)
        lib = _lib.load()
        h = ctx.handle
        c32, ctx.coords, ctx.backward_done = ctx.coords, None, True
        gout = _f32c(gout)
        if h.gacc is None:
            nbytes = int(lib.vsr_raft_corr_workspace_bytes(ctypes.byref(h.desc), 1))
            h.gacc = torch.zeros(nbytes, dtype=torch.uint8, device=gout.device)
        _lib.check(lib.vsr_raft_corr_lookup_bwd(ctypes.byref(h.desc), _ptr(h.packed), h.packed.numel(), _ptr(c32), _ptr(gout),
                                                _ptr(h.gacc), h.gacc.numel(), _stream()), "raft_corr_lookup_bwd")
        return torch.zeros(1, dtype=torch.float32, device=gout.device), None, None


def raft_corr_pyramid(fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int = 4, compute_dtype: Optional[str] = None,
                      radius: int = 3) -> RaftCorrPyramid:
    """Pack ``fmap1`` and build the ``avg_pool2d(2, 2)`` pyramid of ``fmap2`` (both (N, 128, H, W)) once; the returned handle
    serves every ``raft_corr_lookup`` of a forward pass.  Storage is fp32, or bf16 under ``compute_dtype='bf16'`` (fp32
    accumulation either way).  Nothing of size (H W)^2 is ever formed."""
    if fmap1.dim() != 4 or fmap1.shape != fmap2.shape:
        raise ValueError(f"raft_corr_pyramid: fmap1 and fmap2 must have one shape (N, D, H, W); got {tuple(fmap1.shape)} and {tuple(fmap2.shape)}")
    _require_gpu(fmap1, fmap2)
    dtype = resolve_dtype(compute_dtype)
    n, d, h, w = (int(v) for v in fmap1.shape)
    desc = _lib.RaftCorrDesc(n, d, h, w, int(num_levels), int(radius), dtype)
    nbytes = int(_lib.load().vsr_raft_corr_workspace_bytes(ctypes.byref(desc), 0))
    if nbytes == 0:
        raise RuntimeError(_RAFT_UNSUPPORTED.format(shape=tuple(fmap1.shape), levels=num_levels, radius=radius))
    need_bwd = torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad)
    state = _RaftCorrState(desc, torch.empty(nbytes, dtype=torch.uint8, device=fmap1.device), fmap1.shape, int(num_levels), need_bwd)
    return RaftCorrPyramid(state, _RaftPyramidFn.apply(fmap1, fmap2, state))


def raft_corr_lookup(handle: RaftCorrPyramid, coords: torch.Tensor) -> torch.Tensor:
    """(N, num_levels * 49, H, W): channel ``l * 49 + i * 7 + j`` is level ``l`` of the correlation of every pixel with the
    pyramid, sampled bilinearly (zeros outside) at ``coords / 2^l + (i - 3, j - 3)`` -- ``i`` offsets x and ``j`` offsets y, as
    the reference's meshgrid does.  ``coords`` is (N, 2, H, W) with channel 0 = x and receives no gradient; the result is
    differentiable into both maps of the pyramid."""
    n, _, h, w = handle.shape
    if tuple(coords.shape) != (n, 2, h, w):
        raise ValueError(f"raft_corr_lookup: coords must be ({n}, 2, {h}, {w}); got {tuple(coords.shape)}")
    _require_gpu(coords)
    return _RaftLookupFn.apply(handle.token, coords.detach(), handle.state)


def raft_correlation(coords: torch.Tensor, fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int = 4, radius: int = 3,
                     compute_dtype: Optional[str] = None) -> torch.Tensor:
    """The reference's ``correlation(coords, fmap1, fmap2, num_levels, radius)`` in one call: pyramid + one lookup."""
    return raft_corr_lookup(raft_corr_pyramid(fmap1, fmap2, num_levels, compute_dtype, radius=radius), coords)


# --------------------------------------------------------------------------------------------- #
# Local correlation: SpatialCorrelationSampler and PWC's cost volume in one launch
# (reference: core/modules/correlation.py, optical_flow/models/irr/pwc_modules.py:39-59; csrc/spatial_corr.hip,
# built into libvsrlab_spatial_corr.so)
# --------------------------------------------------------------------------------------------- #
_SPATIAL_CORR_UNSUPPORTED = ("vsrlab_amd: spatial_correlation: unsupported shape (patch odd and <= 9, stride 1 or 2, dilation_patch 1 or 2, "
                             "0 <= padding <= dilation_patch * (patch - 1) / 2, each per axis): inputs {shape}, patch_size {patch}, "
                             "stride {stride}, padding {padding}, dilation_patch {dil}")


def _spatial_corr_desc(shape, patch, stride, padding, dil, dtype, scale):
    n, c, h, w = (int(v) for v in shape)
    return _lib.SpatialCorrDesc(n, c, h, w, *patch, *stride, *padding, *dil, int(dtype), float(scale))


def spatial_corr_workspace_bytes(shape, patch_size=1, stride=1, padding=0, dilation_patch=1, dtype: int = DT_F32) -> int:
    """Bytes of the workspace of one ``spatial_correlation`` call on inputs of ``shape`` (N, C, H, W); 0: unsupported.  Host
    arithmetic only."""
    desc = _spatial_corr_desc(shape, _pair(patch_size), _pair(stride), _pair(padding), _pair(dilation_patch), dtype, 1.0)
    return int(_lib.load_spatial_corr().vsr_spatial_corr_workspace_bytes(ctypes.byref(desc)))


class _SpatialCorrFn(torch.autograd.Function):
    """Both gradients are gathers with one owner per element: bit-identical across runs."""

    @staticmethod
    def forward(ctx, input1, input2, cfg):
        desc, nbytes, out_shape, need_bwd = cfg
        lib = _lib.load_spatial_corr()
        a, b = _f32c(input1), _f32c(input2)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        out = torch.empty(out_shape, dtype=torch.float32, device=a.device)
        _lib.check(lib.vsr_spatial_corr_fwd(ctypes.byref(desc), _ptr(a), _ptr(b), _ptr(out), _ptr(ws), nbytes, _stream()), "spatial_corr_fwd")
        del ws
        ctx.desc, ctx.nbytes = desc, nbytes
        ctx.saved = (a, b) if need_bwd else None
        ctx.backward_done = False
        ctx.dtypes = (input1.dtype, input2.dtype)
        return out.to(input1.dtype)

    @staticmethod
    def backward(ctx, gout):
        _backward_once(ctx, "spatial_correlation", ctx.saved is not None)
        (a, b), ctx.saved, ctx.backward_done = ctx.saved, None, True
        gout = _f32c(gout)
        need = ctx.needs_input_grad
        d1 = torch.empty_like(a) if need[0] else None
        d2 = torch.empty_like(b) if need[1] else None
        ws = torch.empty(ctx.nbytes, dtype=torch.uint8, device=a.device)
        _lib.check(_lib.load_spatial_corr().vsr_spatial_corr_bwd(ctypes.byref(ctx.desc), _ptr(a), _ptr(b), _ptr(gout), _ptr(d1), _ptr(d2), _ptr(ws),
                                                    ctx.nbytes, _stream()), "spatial_corr_bwd")
        del ws
        return (None if d1 is None else d1.to(ctx.dtypes[0]), None if d2 is None else d2.to(ctx.dtypes[1]), None)


def spatial_correlation(input1: torch.Tensor, input2: torch.Tensor, patch_size=1, stride=1, padding=0, dilation_patch=1,
                        scale: float = 1.0, compute_dtype: Optional[str] = None) -> torch.Tensor:
    """(N, P_h, P_w, ceil(H' / s_h), ceil(W' / s_w)) in the dtype of ``input1``:
    ``out[n, i, j, y, x] = scale * sum_c in1[n, c, y s_h, x s_w] * in2[n, c, y s_h + i d_h - m_h, x s_w + j d_w - m_w]`` in the
    frame zero-padded by ``padding`` (H' x W'), ``in2`` zero outside it, ``m = dilation_patch * (patch_size - 1) // 2``.  Every
    int-or-pair argument is (vertical, horizontal); ``i`` (slow) is the vertical displacement index.  One kernel launch reads
    each map once; storage is fp32, or bf16 under ``compute_dtype='bf16'`` (fp32 accumulation either way).  Differentiable in
    both inputs.  There is no CPU fallback."""
    if input1.dim() != 4 or input1.shape != input2.shape:
        raise ValueError(f"spatial_correlation: input1 and input2 must have one shape (N, C, H, W); got {tuple(input1.shape)} and {tuple(input2.shape)}")
    patch, strd, pad, dil = _pair(patch_size), _pair(stride), _pair(padding), _pair(dilation_patch)
    if min(patch) < 1 or min(strd) < 1 or min(pad) < 0 or min(dil) < 1 or input1.numel() == 0:
        raise ValueError(f"spatial_correlation: patch_size, stride and dilation_patch must be positive, padding non-negative and the inputs "
                         f"non-empty; got {patch}, {strd}, {dil}, {pad}, {tuple(input1.shape)}")
    dtype = resolve_dtype(compute_dtype)
    desc = _spatial_corr_desc(input1.shape, patch, strd, pad, dil, dtype, scale)
    nbytes = int(_lib.load_spatial_corr().vsr_spatial_corr_workspace_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise RuntimeError(_SPATIAL_CORR_UNSUPPORTED.format(shape=tuple(input1.shape), patch=patch, stride=strd, padding=pad, dil=dil))
    _require_gpu(input1, input2)
    n, _, h, w = (int(v) for v in input1.shape)
    out_shape = (n, patch[0], patch[1], -(-(h + 2 * pad[0]) // strd[0]), -(-(w + 2 * pad[1]) // strd[1]))
    need_bwd = torch.is_grad_enabled() and (input1.requires_grad or input2.requires_grad)
    return _SpatialCorrFn.apply(input1, input2, (desc, nbytes, out_shape, need_bwd))
