"""The whole BasicVSR path as one autograd node (reference: modules/basicvsr.py:39-83 + autograd; csrc/engine.hip), its
workspace and arena mode, then RealBasicVSR's pre-clean stack (reference: vsr/models/RealBasicVSR/realbasicvsr.py:17-30;
csrc/cleaner_engine.hip)."""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import List, Optional, Sequence

import torch

from .. import _lib
from .._lib import BasicVSRDesc
from ._base import _check_width, _f32c, _ptr, _ptr_array, _require_gpu, _stream, resolve_dtype


def _under_ddp() -> bool:
    """True while a torch DistributedDataParallel wrapper is running this forward (DDP's own class-level
    ``_active_ddp_module`` marker, set for the duration of its forward)."""
    try:
        from torch.nn.parallel import DistributedDataParallel
        return getattr(DistributedDataParallel, "_active_ddp_module", None) is not None
    except Exception:
        return False


class Workspace:
    """One arena per forward, owned by that forward's autograd node (``ctx.ws``) until its backward has run or the graph is
    dropped, then returned to PyTorch's caching allocator -- which hands the same block back to the next forward of the same
    size without a hipMalloc, and to anybody else in between (round 2: the GAN iteration needs the generator's 87 GB for the
    discriminator's activations while the generator is idle; a private pool that kept the arena made config 3 run out of
    memory)."""

    def __init__(self, nbytes: int, device):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.owner = None


class WorkspacePool:
    """Allocates arenas and remembers the most recent one WEAKLY (for ``basicvsr_flows``, which reads the flows out of a live
    forward's arena).  It does not keep arenas alive."""

    def __init__(self):
        self._last = None

    def acquire(self, key, nbytes: int, device) -> Workspace:
        ws = Workspace(nbytes, device)
        self._last = weakref.ref(ws)
        return ws

    def last(self) -> Optional[Workspace]:
        return self._last() if self._last is not None else None

    def clear(self):
        self._last = None


class _CtxToken:
    """weakref-able handle tying a workspace to the lifetime of an autograd graph node."""


def _engine_entries(mid_channels: int):
    """The C entries of the BasicVSR engine for a width: vsr_basicvsr_* (64) or vsr_basicvsr_narrow_* (16, 32)."""
    _check_width(mid_channels, "BasicVSR engine")
    lib = _lib.load()
    pre = "vsr_basicvsr_" if mid_channels == 64 else "vsr_basicvsr_narrow_"
    return {k: getattr(lib, pre + k) for k in ("workspace_bytes", "forward", "backward", "get_flows")}


class _BasicVSRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lrs, desc_tuple, pool, n_trainable, need_bwd, direct, *params):
        n, t, h, w, mid, rb, up, dtype, arena = desc_tuple
        desc = BasicVSRDesc(n, t, h, w, mid, rb, up, dtype, arena)
        E = _engine_entries(mid)
        nbytes = E["workspace_bytes"](ctypes.byref(desc), int(need_bwd))
        if nbytes == 0:
            raise RuntimeError(f"vsrlab_amd: unsupported BasicVSR configuration for the HIP path: {desc_tuple}")
        ws = pool.acquire((desc_tuple, need_bwd, lrs.device.index), nbytes, lrs.device)
        lr32 = _f32c(lrs)
        ps = [_f32c(p) for p in params]
        sr = torch.empty((n, t, 3, up * h, up * w), dtype=torch.float32, device=lrs.device)
        _lib.check(E["forward"](ctypes.byref(desc), _ptr_array(ps), len(ps), _ptr(lr32), _ptr(sr), _ptr(ws.buf),
                                ws.buf.numel(), int(need_bwd), _stream()), "basicvsr_forward")
        if need_bwd:
            token = _CtxToken()
            ctx.token = token
            ws.owner = weakref.ref(token)
        ctx.ws = ws
        ctx.desc_tuple = desc_tuple
        ctx.n_trainable = n_trainable
        ctx.need_bwd = need_bwd
        ctx.lr32 = lr32
        ctx.ps = ps
        ctx.direct = direct
        ctx.params = params                 # the leaves themselves: their .grad is re-attached to the arena slot
        ctx.consumed = False
        return sr

    @staticmethod
    def backward(ctx, dsr):
        if not ctx.need_bwd:
            raise RuntimeError("vsrlab_amd: backward through a forward that ran without need_backward")
        if ctx.consumed:
            # the arena went back to the pool after the first backward (a later forward of the same shape may have
            # overwritten the saved activations): fail like PyTorch does for freed buffers instead of returning garbage
            raise RuntimeError("vsrlab_amd: trying to backward through the BasicVSR graph a second time: the saved "
                               "activations live in a pooled workspace that was released by the first backward")
        n, t, h, w, mid, rb, up, dtype, arena = ctx.desc_tuple
        desc = BasicVSRDesc(n, t, h, w, mid, rb, up, dtype, arena)
        ps = ctx.ps
        # need_bwd == 2 (train_flow / input gradient): the SPyNet conv weights / biases (everything but the trailing mean,
        # std buffers) may be differentiated too
        n_diff = len(ps) - 2 if ctx.need_bwd == 2 else ctx.n_trainable
        # Tensors come in (weight, bias) pairs and the engine produces a pair's gradients together: a pair gets slots iff
        # one of its members needs a gradient; everything else is NULL (e.g. all of a frozen SPyNet when only the input
        # clip is differentiated: no 7x7 weight gradient is computed at all).
        need = [k < n_diff and bool(ctx.needs_input_grad[6 + k]) for k in range(len(ps))]
        want = [k < n_diff and (need[k & ~1] or need[k | 1]) for k in range(len(ps))]
        # Gradient destinations.  A parameter managed by vsrlab_amd.optim.FusedAdam carries `_vsr_grad_slot`, a view of
        # the optimizer's flat gradient arena: the engine accumulates (+=) straight into it -- what autograd's
        # AccumulateGrad would do -- and autograd gets None for it.  Everything else goes through ONE zero-filled
        # scratch arena (a fill kernel per tensor costs ~1 ms per step at 254 tensors) and is returned to autograd.
        direct = ctx.direct if ctx.direct is not None else [None] * len(ps)
        sizes = [ps[k].numel() if (want[k] and direct[k] is None) else 0 for k in range(len(ps))]
        offs = [0]
        for sz in sizes:
            offs.append(offs[-1] + ((sz + 63) // 64) * 64)          # 256-byte aligned slots
        flat = torch.zeros(max(offs[-1], 1), dtype=torch.float32, device=dsr.device)
        dest: List[Optional[torch.Tensor]] = []
        for k, p in enumerate(ps):
            if not want[k]:
                dest.append(None)
            elif direct[k] is not None:
                dest.append(direct[k])
            else:
                dest.append(flat[offs[k]:offs[k] + sizes[k]].view(p.shape))
        dlrs = torch.empty_like(ctx.lr32) if ctx.needs_input_grad[0] else None      # gradient w.r.t. the clip (need_bwd == 2)
        _lib.check(_engine_entries(mid)["backward"](ctypes.byref(desc), _ptr_array(ps), _ptr_array(dest), len(ps), _ptr(ctx.lr32),
                                                    _ptr(_f32c(dsr)), _ptr(dlrs), _ptr(ctx.ws.buf), ctx.ws.buf.numel(), _stream()),
                   "basicvsr_backward")
        ctx.consumed = True
        ctx.ws.owner = None
        ctx.ws = None                    # the arena goes back to the allocator now, not when the caller drops the loss tensor
        ctx.token = None
        grads: List[Optional[torch.Tensor]] = []
        for k in range(len(ps)):
            if not need[k]:
                grads.append(None)
            elif direct[k] is not None:
                leaf = ctx.params[k]
                if leaf.grad is None or leaf.grad.data_ptr() != direct[k].data_ptr():
                    leaf.grad = direct[k]                            # e.g. after zero_grad(set_to_none=True)
                grads.append(None)
            else:
                grads.append(dest[k])
        ctx.params = None
        return (dlrs, None, None, None, None, None) + tuple(grads)


_ARENA_MODE: Optional[int] = None


def set_arena_mode(mode: Optional[str]) -> None:
    """Training workspace of the BasicVSR engine (VsrBasicVSRDesc.arena_mode, include/vsrlab_hip.h): "full" (default: every
    activation gradient of a direction kept, all-frames weight-gradient launches; 113 GiB per clip for BASELINE config 2) or "diet" (65 GiB: per-frame
    weight gradients behind a two-block gradient ring, HR activations recomputed; for batch-of-clips per GPU).  None: back to
    $VSRLAB_AMD_ARENA (unset = "full")."""
    global _ARENA_MODE
    if mode is not None and mode not in ("full", "diet"):
        raise ValueError("arena mode is 'full' or 'diet'")
    _ARENA_MODE = None if mode is None else int(mode == "diet")


def arena_mode() -> int:
    if _ARENA_MODE is not None:
        return _ARENA_MODE
    env = os.environ.get("VSRLAB_AMD_ARENA", "full")
    if env not in ("full", "diet"):
        raise ValueError("VSRLAB_AMD_ARENA is 'full' or 'diet'")
    return int(env == "diet")


def basicvsr_forward(lrs: torch.Tensor, params: Sequence[torch.Tensor], n_trainable: int, mid_channels: int,
                     res_blocks: int, upscale: int, pool: WorkspacePool, compute_dtype: Optional[str] = None) -> torch.Tensor:
    """sr = BasicVSR(lrs) on the HIP engine.  ``params`` in state_dict order; the first
    ``n_trainable`` are the non-SPyNet tensors.  SPyNet is frozen unless ``train_flow`` (basicvsr.py:25-28): if any
    of its conv parameters requires grad the engine also keeps SPyNet's activations and differentiates it
    (need_backward = 2)."""
    _require_gpu(lrs)
    if lrs.dim() != 5 or lrs.shape[2] != 3:
        raise ValueError("lrs must be (n,t,3,h,w)")
    _check_width(mid_channels, "BasicVSR engine")
    n, t, _, h, w = lrs.shape
    desc_tuple = (n, t, h, w, mid_channels, res_blocks, upscale, resolve_dtype(compute_dtype), arena_mode())
    # grad mode is off inside Function.forward, so decide here whether activations must be retained
    need_bwd = 0
    if torch.is_grad_enabled():
        if lrs.requires_grad or (t > 1 and any(p.requires_grad for p in params[n_trainable:])):
            need_bwd = 2                                      # input-clip and / or SPyNet gradients: SPyNet's activations are kept
        elif any(p.requires_grad for p in params[:n_trainable]):
            need_bwd = 1
    # parameters owned by vsrlab_amd.optim.FusedAdam receive their gradient in place (see _BasicVSRFn.backward);
    # under DistributedDataParallel the gradients must flow through autograd so that DDP's hooks fire
    direct = [getattr(p, "_vsr_grad_slot", None) if (p.requires_grad and not _under_ddp()) else None for p in params]
    if not any(d is not None for d in direct):
        direct = None
    return _BasicVSRFn.apply(lrs, desc_tuple, pool, n_trainable, need_bwd, direct, *params)


def basicvsr_flows(lrs_shape, mid_channels, res_blocks, upscale, ws: Workspace, dtype: int, device):
    n, t, _, h, w = lrs_shape
    desc = BasicVSRDesc(n, t, h, w, mid_channels, res_blocks, upscale, dtype)
    ff = torch.empty((n, t - 1, 2, h, w), dtype=torch.float32, device=device)
    fb = torch.empty_like(ff)
    _lib.check(_engine_entries(mid_channels)["get_flows"](ctypes.byref(desc), _ptr(ws.buf), _ptr(ff), _ptr(fb), _stream()), "get_flows")
    return ff, fb


# --------------------------------------------------------------------------------------------- #
# RealBasicVSR pre-clean stack, forward (reference: vsr/models/RealBasicVSR/realbasicvsr.py:17-30)
# --------------------------------------------------------------------------------------------- #
class _CleanerFn(torch.autograd.Function):
    """lq = IterativeRefinement(lr) with its backward on the HIP engine (parameter gradients and d lr)."""

    @staticmethod
    def forward(ctx, lr, meta, *params):
        mid_channels, blocks, steps, dtype, need_bwd = meta
        n, t, _, h, w = lr.shape
        lib = _lib.load()
        ps = [_f32c(p) for p in params]
        lr32 = _f32c(lr)
        if mid_channels == 64:
            nbytes = lib.vsr_cleaner_workspace_bytes(n * t, h, w, blocks, steps, dtype, int(need_bwd))
        else:
            nbytes = lib.vsr_cleaner_narrow_workspace_bytes(n * t, h, w, mid_channels, blocks, steps, dtype, int(need_bwd))
        if nbytes == 0:
            raise RuntimeError("vsrlab_amd: unsupported pre-clean configuration for the HIP path")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=lr.device)
        lq = torch.empty((n, t, 3, h, w), dtype=torch.float32, device=lr.device)
        _lib.check(lib.vsr_cleaner_forward(n * t, h, w, mid_channels, blocks, steps, dtype, _ptr_array(ps), len(ps), _ptr(lr32),
                                           _ptr(lq), _ptr(ws), ws.numel(), int(need_bwd), _stream()), "cleaner_forward")
        ctx.meta = meta
        ctx.ws = ws if need_bwd else None
        ctx.lr32 = lr32 if need_bwd else None
        ctx.shapes = [p.shape for p in ps]
        return lq

    @staticmethod
    def backward(ctx, dlq):
        mid_channels, blocks, steps, dtype, need_bwd = ctx.meta
        if not need_bwd:
            raise RuntimeError("vsrlab_amd: backward through a pre-clean forward that ran without need_backward")
        if ctx.ws is None:
            raise RuntimeError("vsrlab_amd: trying to backward through the pre-clean graph a second time")
        n, t, _, h, w = dlq.shape
        lib = _lib.load()
        grads = [torch.zeros(sh, dtype=torch.float32, device=dlq.device) for sh in ctx.shapes]
        dlr = torch.empty_like(ctx.lr32) if ctx.needs_input_grad[0] else None
        _lib.check(lib.vsr_cleaner_backward(n * t, h, w, mid_channels, blocks, steps, dtype, _ptr_array(grads), len(grads),
                                            _ptr(ctx.lr32), _ptr(_f32c(dlq)), _ptr(dlr), _ptr(ctx.ws), ctx.ws.numel(), _stream()),
                   "cleaner_backward")
        ctx.ws = None
        return (dlr, None) + tuple(g if ctx.needs_input_grad[2 + k] else None for k, g in enumerate(grads))


def cleaner_forward(params: Sequence[torch.Tensor], lr: torch.Tensor, mid_channels: int, blocks: int, steps: int = 3,
                    compute_dtype: Optional[str] = None) -> torch.Tensor:
    """lq = IterativeRefinement(lr): (n,t,3,h,w) -> (n,t,3,h,w), a fresh tensor (the reference adds in place,
    realbasicvsr.py:29).  Differentiable w.r.t. the parameters and lr."""
    _require_gpu(lr)
    if len(params) != 4 + 4 * blocks:
        raise ValueError("expected the 4 + 4*blocks tensors of IterativeRefinement")
    n, t, c, h, w = lr.shape
    if c != 3:
        raise ValueError("lr must be (n,t,3,h,w)")
    _check_width(mid_channels, "pre-clean stack")
    need_bwd = torch.is_grad_enabled() and (lr.requires_grad or any(p.requires_grad for p in params))
    return _CleanerFn.apply(lr, (mid_channels, blocks, steps, resolve_dtype(compute_dtype), need_bwd), *params)
