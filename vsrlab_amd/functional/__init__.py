"""torch-facing wrappers over the C ABI: PyTorch supplies device memory, the current HIP stream
and autograd bookkeeping; every FLOP runs in the HIP libraries that ``_lib`` loads.

There is deliberately no CPU / eager fallback: a tensor that is not on a GPU raises.

One submodule per op family; this file only re-exports, so ``from vsrlab_amd import functional as VF`` keeps every name.
Callers look entry points up on the package at call time (``VF.basicvsr_forward(...)``).  A helper such as ``_require_gpu`` is
bound in each submodule that calls it: patch it there."""
# flake8: noqa: F401
from . import basicvsr, conv
from .._lib import BasicVSRDesc, DT_BF16, DT_F32
from ._base import (
    MID_CHANNELS, _DT, _STORAGE_DT, _TORCH_DT, _backward_once, _check_width, _f32c, _pair, _ptr, _ptr_array,
    _require_gpu, _stream, resolve_dtype)
from .layout import _pm_dims, _pm_like, from_pixel_major, to_pixel_major
from .warp import (
    _AlignedInputFn, _FlowWarpFn, _WarpTapsFn, _flow_f32, _warp_taps, _warp_taps_checks, _warp_taps_desc,
    aligned_input, flow_warp)
from .conv import (
    ResidualChainC64, _ConvLayerFn, _ResidualConvFn, _conv_layer_autograd, chain_timeouts, conv3x3_c64,
    conv3x3_c64_dgrad, conv3x3_c64_wgrad, conv_layer, conv_relu_forward, pixel_shuffle_pack_forward,
    raise_on_chain_timeout, residual_block_forward, residual_conv)
from .spynet import _SpynetFn, _SpynetLevelsFn, spynet_flow, spynet_levels, spynet_module_forward
from .basicvsr import (
    Workspace, WorkspacePool, _BasicVSRFn, _CleanerFn, _CtxToken, _engine_entries, _under_ddp, arena_mode,
    basicvsr_flows, basicvsr_forward, cleaner_forward, set_arena_mode)
from .gan import (
    DEFAULT_PERCEPTUAL_WORKSPACE, PERCEPTUAL_LAYER_WEIGHTS, VGG19_CONVS, _BCEFn, _CharbonnierFn, _DISC_SPECTRAL,
    _DiscriminatorFn, _PerceptualFn, _SpectralNormFn, _TAP_CHANNELS, _TAP_LEVELS, _perceptual_desc, _tap_numels,
    bce_with_logits_const, charbonnier_loss, discriminator_forward, perceptual_chunk, perceptual_loss,
    perceptual_workspace_bytes, spectral_conv_forward)
from .attention import _MASK_BITS, _WindowAttentionFn, _packed_mask, window_attention_core
from .deform import (
    _DeformConvFn, _deform_checks, _deform_desc, deform_conv2d, deform_conv_workspace_bytes,
    flow_guided_deform_conv, flow_guided_offset_mask)
from .metrics import PsnrSsimSums, psnr_ssim
from .correlation import (
    RaftCorrPyramid, _RAFT_UNSUPPORTED, _RaftCorrState, _RaftLookupFn, _RaftPyramidFn, _SPATIAL_CORR_UNSUPPORTED,
    _SpatialCorrFn, _spatial_corr_desc, raft_corr_lookup, raft_corr_pyramid, raft_corr_workspace_bytes,
    raft_correlation, spatial_corr_workspace_bytes, spatial_correlation)
from .jpeg import jpeg_compress


def __getattr__(name):
    """The two globals that their functions rebind are read where they live, never copied: ``_ARENA_MODE`` (set_arena_mode)
    in ``basicvsr``, ``_chain_timeouts_seen`` (raise_on_chain_timeout) in ``conv``."""
    if name == "_ARENA_MODE":
        return basicvsr._ARENA_MODE
    if name == "_chain_timeouts_seen":
        return conv._chain_timeouts_seen
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
