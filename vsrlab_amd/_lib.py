"""ctypes binding of the C ABI in include/vsrlab_hip.h (lib/libvsrlab_hip.so).

The product path has no fallback: if the HIP library is missing or a call returns a non-zero
status, a RuntimeError is raised.
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# VSRLAB_AMD_LIB: another build of the same library (the clock build `make CLOCK=1`, or a parent commit's), for whole-step A/B runs
LIB_PATH = os.environ.get("VSRLAB_AMD_LIB") or os.path.join(_HERE, "lib", "libvsrlab_hip.so")

DT_F32 = 0
DT_BF16 = 1


class BasicVSRDesc(ctypes.Structure):
    """struct VsrBasicVSRDesc (include/vsrlab_hip.h)."""
    _fields_ = [("n", c_int), ("t", c_int), ("h", c_int), ("w", c_int), ("mid_channels", c_int),
                ("res_blocks", c_int), ("upscale", c_int), ("dtype", c_int), ("arena_mode", c_int)]


class DiscDesc(ctypes.Structure):
    """struct VsrDiscDesc (include/vsrlab_hip.h)."""
    _fields_ = [("n", c_int), ("h", c_int), ("w", c_int), ("mid_ch", c_int), ("dtype", c_int)]


class PerceptualDesc(ctypes.Structure):
    """struct VsrPerceptualDesc (include/vsrlab_hip.h)."""
    _fields_ = [("n", c_int), ("h", c_int), ("w", c_int), ("dtype", c_int), ("need_grad", c_int)]


class AttnDesc(ctypes.Structure):
    """struct VsrAttnDesc (include/vsrlab_hip.h)."""
    _fields_ = [(k, c_int) for k in ("B", "N", "heads", "head_dim", "q0", "k0", "o0", "Nq", "Nk", "Cout", "c_off", "nW", "Nm")] + \
               [("scale", c_float), ("dtype", c_int), ("mask_packed", c_int), ("mask_value", c_float)]


class DeformDesc(ctypes.Structure):
    """struct VsrDeformDesc (include/vsrlab_hip.h)."""
    _fields_ = [(k, c_int) for k in ("N", "Cin", "Cout", "H", "W", "deform_groups", "modulated", "flow_guided")] + \
               [("max_residue", c_float), ("dtype", c_int)]


class MetricsDesc(ctypes.Structure):
    """struct VsrMetricsDesc (include/vsrlab_hip.h)."""
    _fields_ = [("planes", c_longlong), ("C", c_int), ("H", c_int), ("W", c_int), ("window_size", c_int),
                ("sigma", c_float), ("c1", c_float), ("c2", c_float), ("clamp_x", c_int), ("clamp_lo", c_float), ("clamp_hi", c_float)]


class RaftCorrDesc(ctypes.Structure):
    """struct VsrRaftCorrDesc (include/vsrlab_hip.h)."""
    _fields_ = [(k, c_int) for k in ("N", "D", "H", "W", "levels", "radius", "dtype")]


class SpatialCorrDesc(ctypes.Structure):
    """struct VsrSpatialCorrDesc (include/vsrlab_spatial_corr.h)."""
    _fields_ = [(k, c_int) for k in ("N", "C", "H", "W", "patch_h", "patch_w", "stride_h", "stride_w", "pad_h", "pad_w", "dil_h", "dil_w",
                                     "dtype")] + [("scale", c_float)]


class JpegDesc(ctypes.Structure):
    """struct VsrJpegDesc (include/vsrlab_jpeg.h)."""
    _fields_ = [(k, c_int) for k in ("N", "H", "W", "quality", "x_dtype", "y_dtype")] + \
               [("x_stride", c_longlong * 4), ("y_stride", c_longlong * 4)]


class WarpTapsDesc(ctypes.Structure):
    """struct VsrWarpTapsDesc (include/vsrlab_warp_taps.h)."""
    _fields_ = [(k, c_int) for k in ("N", "D", "C", "H", "W", "taps", "border", "dtype")] + [("x_nstride", c_longlong)]


class BlockDctDesc(ctypes.Structure):
    """struct VsrBlockDctDesc (include/vsrlab_mixer.h)."""
    _fields_ = [(k, c_int) for k in ("N", "C", "H", "W", "ps", "dtype")]


class AxisMlpDesc(ctypes.Structure):
    """struct VsrAxisMlpDesc (include/vsrlab_mixer.h)."""
    _fields_ = [("outer", c_longlong), ("D", c_int), ("inner", c_longlong), ("hidden", c_int), ("dtype", c_int), ("residual", c_int)]


class Conv3dDesc(ctypes.Structure):
    """struct VsrConv3dDesc (include/vsrlab_conv3d.h)."""
    _fields_ = [(k, c_int) for k in ("B", "Cin", "Cout", "T", "H", "W", "taps", "dtype", "act")] + \
               [("slope", c_float), ("pixel_shuffle", c_int), ("x_stride", c_longlong * 3), ("y_stride", c_longlong * 3)]


_P = c_void_p
_SIGNATURES = {
    "vsr_abi_version": (c_int, []),
    "vsr_status_string": (c_char_p, [c_int]),
    "vsr_basicvsr_num_params": (c_int, [ctypes.POINTER(BasicVSRDesc)]),
    "vsr_basicvsr_workspace_bytes": (c_size_t, [ctypes.POINTER(BasicVSRDesc), c_int]),
    "vsr_basicvsr_forward": (c_int, [ctypes.POINTER(BasicVSRDesc), _P, c_int, _P, _P, _P, c_size_t, c_int, _P]),
    "vsr_basicvsr_backward": (c_int, [ctypes.POINTER(BasicVSRDesc), _P, _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_basicvsr_get_flows": (c_int, [ctypes.POINTER(BasicVSRDesc), _P, _P, _P, _P]),
    "vsr_basicvsr_narrow_workspace_bytes": (c_size_t, [ctypes.POINTER(BasicVSRDesc), c_int]),
    "vsr_basicvsr_narrow_forward": (c_int, [ctypes.POINTER(BasicVSRDesc), _P, c_int, _P, _P, _P, c_size_t, c_int, _P]),
    "vsr_basicvsr_narrow_backward": (c_int, [ctypes.POINTER(BasicVSRDesc), _P, _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_basicvsr_narrow_get_flows": (c_int, [ctypes.POINTER(BasicVSRDesc), _P, _P, _P, _P]),
    "vsr_spynet_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "vsr_spynet_forward": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P, c_size_t, c_int, _P]),
    "vsr_spynet_backward": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_size_t, _P]),
    "vsr_spynet_forward_ex": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, _P, c_size_t, c_int, _P]),
    "vsr_spynet_backward_ex": (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_cleaner_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "vsr_cleaner_narrow_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "vsr_cleaner_forward": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, c_size_t, c_int, _P]),
    "vsr_cleaner_backward": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_flow_warp_fwd": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_flow_warp_bwd": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_flow_warp_bwd_flow": (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_flow_warp_fwd_ex": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_flow_warp_bwd_ex": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_flow_warp_bwd_flow_ex": (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_planar_to_pm": (c_int, [c_int, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_pm_to_planar": (c_int, [c_int, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_conv3x3_c64_fwd": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_conv3x3_c64_chain_sync_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "vsr_conv3x3_c64_chain_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "vsr_conv3x3_c64_dgrad": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_conv_layer_fwd": (c_int, [c_int, c_int, _P, c_int, _P, _P, _P, c_int, c_int, _P, _P, c_int, _P, c_int, c_float, c_int, c_int, c_int, c_int, _P]),
    "vsr_conv_layer_bwd_scratch_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "vsr_conv_layer_bwd": (c_int, [c_int, c_int, _P, c_int, _P, _P, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_float, c_int, _P, _P, _P, _P,
                                   _P, c_size_t, c_int, c_int, c_int, _P]),
    "vsr_conv3x3_c64_wgrad_slab_floats": (c_size_t, []),
    "vsr_conv3x3_c64_wgrad": (c_int, [c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_charbonnier_scratch_floats": (c_size_t, []),
    "vsr_charbonnier_fwd_bwd": (c_int, [_P, _P, _P, _P, _P, c_longlong, c_float, _P]),
    "vsr_optim_scratch_floats": (c_size_t, []),
    "vsr_adam_clip_step": (c_int, [_P, _P, _P, _P, c_longlong, c_float, c_float, c_float, c_float, c_float, c_int, c_float,
                                   c_float, _P, _P, _P]),
    "vsr_grad_norm": (c_int, [_P, c_longlong, c_float, _P, _P, _P]),
    "vsr_resize_bilinear": (c_int, [_P, _P, c_longlong, c_int, c_int, c_int, c_int, _P]),
    "vsr_disc_workspace_bytes": (c_size_t, [ctypes.POINTER(DiscDesc), c_int]),
    "vsr_disc_forward": (c_int, [ctypes.POINTER(DiscDesc), _P, c_int, _P, _P, _P, c_size_t, c_int, _P]),
    "vsr_disc_backward": (c_int, [ctypes.POINTER(DiscDesc), _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_spectral_norm": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_spectral_norm_backward": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, _P, _P]),
    "vsr_bce_with_logits": (c_int, [_P, c_float, _P, _P, c_longlong, _P]),
    "vsr_perceptual_workspace_bytes": (c_size_t, [ctypes.POINTER(PerceptualDesc)]),
    "vsr_perceptual_loss": (c_int, [ctypes.POINTER(PerceptualDesc), _P, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_window_attention_fwd": (c_int, [ctypes.POINTER(AttnDesc), _P, _P, _P, _P, _P, _P]),
    "vsr_window_attention_bwd": (c_int, [ctypes.POINTER(AttnDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "vsr_mask_pack": (c_int, [_P, _P, c_int, c_int, _P]),
    "vsr_rpb_gather": (c_int, [_P, _P, c_int, _P, c_int, c_int, _P]),
    "vsr_rpb_scatter": (c_int, [_P, _P, c_int, _P, c_int, c_int, _P]),
    "vsr_deform_conv_workspace_bytes": (c_size_t, [ctypes.POINTER(DeformDesc), c_int]),
    "vsr_deform_conv_fwd": (c_int, [ctypes.POINTER(DeformDesc), _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_deform_conv_bwd": (c_int, [ctypes.POINTER(DeformDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_deform_offset_mask": (c_int, [ctypes.POINTER(DeformDesc), _P, _P, _P, _P, _P]),
    "vsr_metrics_scratch_bytes": (c_size_t, [ctypes.POINTER(MetricsDesc)]),
    "vsr_psnr_ssim": (c_int, [ctypes.POINTER(MetricsDesc), _P, _P, _P, _P, c_size_t, _P]),
    "vsr_raft_corr_workspace_bytes": (c_size_t, [ctypes.POINTER(RaftCorrDesc), c_int]),
    "vsr_raft_corr_pyramid_fwd": (c_int, [ctypes.POINTER(RaftCorrDesc), _P, _P, _P, c_size_t, _P]),
    "vsr_raft_corr_pyramid_bwd": (c_int, [ctypes.POINTER(RaftCorrDesc), _P, c_size_t, _P, _P, _P]),
    "vsr_raft_corr_lookup_fwd": (c_int, [ctypes.POINTER(RaftCorrDesc), _P, c_size_t, _P, _P, _P]),
    "vsr_raft_corr_lookup_bwd": (c_int, [ctypes.POINTER(RaftCorrDesc), _P, c_size_t, _P, _P, _P, c_size_t, _P]),
}
EXPORTS = tuple(_SIGNATURES)

# Test hooks of csrc/hr_tail_hooks.hip, trunk_hooks.hip, spynet_hooks.hip, wide_hooks.hip and warp_hooks.hip: exported by the library, not part of include/vsrlab_hip.h (so not in
# EXPORTS, like the other vsr_debug_* entries, whose argument types the tests that call them set by hand).  These fourteen have long
# mixed int / long long / float / pointer lists and three callers each (a host test, a GPU test, the driver), so their types are stated
# once, here; load() applies them.  csrc/debug_hooks.h declares every hook once for the compiler, and tests/test_host_logic.py holds
# these rows to it, position by position.
# OTHER_DEBUG_EXPORTS: the library's remaining vsr_debug_* symbols.  EXPORTS + OTHER_DEBUG_EXPORTS + DEBUG_SIGNATURES is every
# `vsr_` symbol the product library exports (tests/test_hr_tail_host.py enumerates its dynamic symbol table against this).
OTHER_DEBUG_EXPORTS = ("vsr_debug_chain_inject_error", "vsr_debug_chain_item", "vsr_debug_chain_timeouts", "vsr_debug_chain_timing_begin",
                       "vsr_debug_chain_timing_read", "vsr_debug_warp_bwd_gather", "vsr_debug_warp_bwd_gather_c")
_LL = c_longlong
DEBUG_SIGNATURES = {
    "vsr_debug_tail_last2_fwd": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _LL, _P, _P, _LL, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_tail_last2_dgrad": (c_int, [_P, _LL, _P, _P, c_int, _P, c_int, c_float, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_tail_planar_c64": (c_int, [c_int, _P, _LL, c_int, _P, _P, _P, _P, c_int, c_float, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_tail_last2_wgrad": (c_int, [c_int, _P, _P, _LL, c_int, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_tail_conv_unshuffle": (c_int, [c_int, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_tail_ps_dgrad": (c_int, [c_int, _P, _P, _P, _P, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_tail_ps_wgrads": (c_int, [c_int, _P, _P, c_int, _P, _P, _P, c_int, c_int, c_int, _P]),
    # csrc/trunk_hooks.hip (dtype, C first; the weight-gradient and chain entries take HOST arrays of device pointers / layer words)
    "vsr_debug_trunk_conv": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, c_float, _P, _P, c_int, _P, _P, c_int, c_int,
                                     c_int, c_int, c_int, _P]),
    "vsr_debug_trunk_stem": (c_int, [c_int, c_int, c_int, _P, _P, _LL, _P, _P, _P, _P, c_int, c_float, c_int, c_int, c_int, _P]),
    "vsr_debug_trunk_stem_dgrad": (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _LL, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_trunk_point": (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_trunk_wgrad_cc": (c_int, [c_int, c_int, c_int, _P, _P, c_int, _P, c_int, c_int, _P, c_int, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_trunk_stem_wgrads": (c_int, [c_int, c_int, c_int, _P, _LL, _P, c_int, _P, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_trunk_chain": (c_int, [c_int, c_int, _P, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, _P]),
    # csrc/spynet_hooks.hip (dtype, layer j first for the three 7x7 entries; vsr_debug_spy_planar: op first, `planes` a long long)
    "vsr_debug_spy_conv": (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_spy_dgrad": (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_spy_wgrad": (c_int, [c_int, c_int, _P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_spy_prepare": (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_spy_prepare_bwd": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_spy_dres": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_spy_planar": (c_int, [c_int, _P, _P, _P, _P, _P, _LL, c_int, c_int, c_int, c_int, _P]),
    # csrc/wide_hooks.hip (dtype first; vsr_debug_wide_conv: mode, cout, cin next, wpack_elems and slab_floats are long long), the plan
    # hook of csrc/disc_engine.hip and the two host-only grid entries (csrc/conv_wide.hip's cap setter; the grid of a conv_wide2 launch)
    "vsr_debug_wide_conv": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P, _P, _LL, _P, c_int, c_float, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_wide_wgrad": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P, _P, _LL, c_int, c_int, c_int, _P]),
    "vsr_debug_wide_up2_fwd": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_wide_up2_bwd": (c_int, [c_int, _P, _P, _P, _P, c_float, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_wide_mask": (c_int, [c_int, _P, _P, _P, c_float, _LL, _P]),
    "vsr_debug_vgg_pool": (c_int, [c_int, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_vgg_tap": (c_int, [c_int, _P, _P, c_int, c_float, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_disc_plan": (c_int, [ctypes.POINTER(DiscDesc), c_int, _P, c_int]),
    "vsr_debug_wide_grid": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_wide2_set_max_wg": (c_int, [c_int]),
    # csrc/warp_hooks.hip (dtype, C first; flow_nstride, a long long, follows the flow pointer)
    "vsr_debug_warp_fwd": (c_int, [c_int, c_int, _P, _P, _LL, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_warp_scatter": (c_int, [c_int, c_int, _P, _P, _LL, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_warp_gather": (c_int, [c_int, c_int, _P, _P, _LL, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "vsr_debug_warp_flowgrad": (c_int, [c_int, c_int, _P, _P, _P, _LL, _P, c_int, c_int, c_int, c_int, _P]),
    "vsr_debug_warp_add_cast": (c_int, [c_int, c_int, _P, _P, _P, c_int, c_int, c_int, _P]),
}

# libvsrlab_spatial_corr.so (include/vsrlab_spatial_corr.h): the local correlation, a library of its own -- the symbols that
# libvsrlab_hip.so exports are pinned and stay as they are
SPATIAL_CORR_LIB_PATH = os.path.join(_HERE, "lib", "libvsrlab_spatial_corr.so")
SPATIAL_CORR_SIGNATURES = {
    "vsr_spatial_corr_workspace_bytes": (c_size_t, [ctypes.POINTER(SpatialCorrDesc)]),
    "vsr_spatial_corr_fwd": (c_int, [ctypes.POINTER(SpatialCorrDesc), _P, _P, _P, _P, c_size_t, _P]),
    "vsr_spatial_corr_bwd": (c_int, [ctypes.POINTER(SpatialCorrDesc), _P, _P, _P, _P, _P, _P, c_size_t, _P]),
}
SPATIAL_CORR_EXPORTS = tuple(SPATIAL_CORR_SIGNATURES)

# libvsrlab_jpeg.so (include/vsrlab_jpeg.h): the JPEG round trip, a library of its own for the same reason
JPEG_LIB_PATH = os.path.join(_HERE, "lib", "libvsrlab_jpeg.so")
JPEG_SIGNATURES = {
    "vsr_jpeg_workspace_bytes": (c_size_t, [ctypes.POINTER(JpegDesc)]),
    "vsr_jpeg_fwd": (c_int, [ctypes.POINTER(JpegDesc), _P, _P, _P, c_size_t, _P]),
}
JPEG_EXPORTS = tuple(JPEG_SIGNATURES)

# libvsrlab_warp_taps.so (include/vsrlab_warp_taps.h): the integer-tap warps ('nearest', 'nearest4') and VRT's aligned input, likewise
WARP_TAPS_LIB_PATH = os.path.join(_HERE, "lib", "libvsrlab_warp_taps.so")
WARP_TAPS_SIGNATURES = {
    "vsr_warp_taps_fwd": (c_int, [ctypes.POINTER(WarpTapsDesc), _P, _P, _P, _P]),
    "vsr_warp_taps_bwd": (c_int, [ctypes.POINTER(WarpTapsDesc), _P, _P, _P, _P, _P]),
    "vsr_warp_taps_clip_fwd": (c_int, [ctypes.POINTER(WarpTapsDesc), _P, _P, _P, _P, _P]),
    "vsr_warp_taps_clip_bwd": (c_int, [ctypes.POINTER(WarpTapsDesc), _P, _P, _P, _P, _P, _P]),
}
WARP_TAPS_EXPORTS = tuple(WARP_TAPS_SIGNATURES)

# libvsrlab_losses.so (include/vsrlab_losses.h): the pair reductions of WL1Loss / rmse_loss and the adjoint of the bilinear resize, likewise
LOSSES_LIB_PATH = os.path.join(_HERE, "lib", "libvsrlab_losses.so")
LOSS_L1 = 0
LOSS_MSE = 1
LOSSES_SIGNATURES = {
    "vsr_pixel_loss_scratch_floats": (c_size_t, []),
    "vsr_pixel_loss_fwd_bwd": (c_int, [c_int, _P, c_int, _P, c_int, _P, _P, _P, c_longlong, _P]),
    "vsr_resize_bilinear_bwd": (c_int, [_P, _P, c_longlong, c_int, c_int, c_int, c_int, _P]),
}
LOSSES_EXPORTS = tuple(LOSSES_SIGNATURES)

# libvsrlab_mixer.so (include/vsrlab_mixer.h): the block DCT and the residual axis MLP of the DCT-token MLP-Mixer, likewise
MIXER_LIB_PATH = os.path.join(_HERE, "lib", "libvsrlab_mixer.so")
AXIS_MLP_MAX_D = 48
AXIS_MLP_MAX_HIDDEN = 1024
MIXER_SIGNATURES = {
    "vsr_block_dct_fwd": (c_int, [ctypes.POINTER(BlockDctDesc), _P, _P, _P, _P]),
    "vsr_block_idct_fwd": (c_int, [ctypes.POINTER(BlockDctDesc), _P, _P, _P, _P]),
    "vsr_axis_mlp_supported": (c_int, [ctypes.POINTER(AxisMlpDesc)]),
    "vsr_axis_mlp_scratch_bytes": (c_size_t, [ctypes.POINTER(AxisMlpDesc)]),
    "vsr_axis_mlp_fwd": (c_int, [ctypes.POINTER(AxisMlpDesc), _P, _P, _P, _P, _P, _P, _P]),
    "vsr_axis_mlp_bwd": (c_int, [ctypes.POINTER(AxisMlpDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
}
MIXER_EXPORTS = tuple(MIXER_SIGNATURES)

# libvsrlab_conv3d.so (include/vsrlab_conv3d.h): the planar, strided Conv3d of ConvST, PixelShufflePack3D and VRT's Upsample, likewise
CONV3D_LIB_PATH = os.path.join(_HERE, "lib", "libvsrlab_conv3d.so")
CONV3D_133, CONV3D_311, CONV3D_333 = 0, 1, 2
CONV3D_ACT_NONE, CONV3D_ACT_LEAKY = 0, 1
CONV3D_MAX_C = 256
CONV3D_SIGNATURES = {
    "vsr_conv3d_workspace_bytes": (c_size_t, [ctypes.POINTER(Conv3dDesc), c_int]),
    "vsr_conv3d_fwd": (c_int, [ctypes.POINTER(Conv3dDesc), _P, _P, _P, _P, _P, c_size_t, _P]),
    "vsr_conv3d_bwd": (c_int, [ctypes.POINTER(Conv3dDesc), _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
}
CONV3D_EXPORTS = tuple(CONV3D_SIGNATURES)

# One row per library: its path, the signatures of its ABI, and those of its debug hooks, which only a library that VSRLAB_AMD_LIB
# names (another build of libvsrlab_hip.so, e.g. a parent commit's for an A/B run) may predate.  _loaded: one slot per library.
_LIBS = {
    "hip": (LIB_PATH, _SIGNATURES, DEBUG_SIGNATURES),
    "spatial_corr": (SPATIAL_CORR_LIB_PATH, SPATIAL_CORR_SIGNATURES, {}),
    "jpeg": (JPEG_LIB_PATH, JPEG_SIGNATURES, {}),
    "warp_taps": (WARP_TAPS_LIB_PATH, WARP_TAPS_SIGNATURES, {}),
    "losses": (LOSSES_LIB_PATH, LOSSES_SIGNATURES, {}),
    "mixer": (MIXER_LIB_PATH, MIXER_SIGNATURES, {}),
    "conv3d": (CONV3D_LIB_PATH, CONV3D_SIGNATURES, {}),
}
_loaded = {}


def _load(key):
    """Load a library (once) and set the types of its entries.  Raises RuntimeError if it has not been built: a missing kernel is an
    error."""
    if key not in _loaded:
        path, signatures, hooks = _LIBS[key]
        if not os.path.exists(path):
            raise RuntimeError(
                f"vsrlab_amd: HIP library not built ({path} missing). Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C vsrlab_amd/csrc`.")
        lib = ctypes.CDLL(path)
        may_lack = hooks if os.environ.get("VSRLAB_AMD_LIB") else {}
        for name, (res, args) in {**signatures, **hooks}.items():
            # AttributeError if the ABI lost a symbol, or the project's own build a hook
            fn = getattr(lib, name, None) if name in may_lack else getattr(lib, name)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        _loaded[key] = lib
    return _loaded[key]


def load():
    """libvsrlab_hip.so."""
    return _load("hip")


def load_spatial_corr():
    """libvsrlab_spatial_corr.so."""
    return _load("spatial_corr")


def load_jpeg():
    """libvsrlab_jpeg.so."""
    return _load("jpeg")


def load_warp_taps():
    """libvsrlab_warp_taps.so."""
    return _load("warp_taps")


def load_losses():
    """libvsrlab_losses.so."""
    return _load("losses")


def load_mixer():
    """libvsrlab_mixer.so."""
    return _load("mixer")


def load_conv3d():
    """libvsrlab_conv3d.so."""
    return _load("conv3d")


def check(status, what):
    if status != 0:
        msg = load().vsr_status_string(status).decode()
        raise RuntimeError(f"vsrlab_amd: {what} failed: {msg} (status {status})")
