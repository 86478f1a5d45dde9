"""CPU tests of the narrow-width entries (mid_channels 16 / 32, vsr_basicvsr_narrow_*, vsr_cleaner_narrow_workspace_bytes):
workspace queries, rejected widths and shapes, and the no-CPU-fallback rule.  No GPU compute is called."""
import ctypes

import pytest
import torch


def _q(lib, fn, mid, rb=30, up=4, arena=0, nb=1, dtype=1):
    from vsrlab_amd import _lib
    d = _lib.BasicVSRDesc(1, 7, 540, 960, mid, rb, up, dtype, arena)
    return getattr(lib, fn)(ctypes.byref(d), nb)


def test_narrow_workspace_query_is_positive_and_scales_with_the_width():
    from vsrlab_amd import _lib
    lib = _lib.load()
    for arena in (0, 1):
        for nb in (0, 1, 2):
            for up in (2, 4):
                q16 = _q(lib, "vsr_basicvsr_narrow_workspace_bytes", 16, up=up, arena=arena, nb=nb)
                q32 = _q(lib, "vsr_basicvsr_narrow_workspace_bytes", 32, up=up, arena=arena, nb=nb)
                q64 = _q(lib, "vsr_basicvsr_workspace_bytes", 64, up=up, arena=arena, nb=nb)
                assert 0 < q16 < q32 < q64, (arena, nb, up, q16, q32, q64)
    # diet is smaller than full when training; inference ignores the arena mode
    for mid in (16, 32):
        full = _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, arena=0)
        diet = _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, arena=1)
        assert 0 < diet < full
        assert _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, arena=0, nb=0) == \
            _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, arena=1, nb=0)


def test_narrow_entries_reject_other_widths_and_shapes():
    from vsrlab_amd import _lib
    lib = _lib.load()
    for mid in (8, 24, 48, 64, 128):
        for nb in (0, 1, 2):
            assert _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, nb=nb) == 0, (mid, nb)
    for mid in (16, 32):
        assert _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, up=3) == 0
        assert _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, rb=0) == 0
        assert _q(lib, "vsr_basicvsr_narrow_workspace_bytes", mid, dtype=2) == 0
        # the whole-path query keeps its contract: 64 only
        assert _q(lib, "vsr_basicvsr_workspace_bytes", mid) == 0
        d = _lib.BasicVSRDesc(1, 7, 540, 960, mid, 30, 4, 1)
        # a rejected width fails before any pointer is touched
        assert lib.vsr_basicvsr_narrow_forward(ctypes.byref(d), None, 0, None, None, None, 0, 0, None) == -1
    d = _lib.BasicVSRDesc(1, 2, 16, 16, 64, 2, 4, 1)
    buf = ctypes.create_string_buffer(16)
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    assert lib.vsr_basicvsr_narrow_forward(ctypes.byref(d), ptrs, 1, ptrs[0], ptrs[0], ptrs[0], 16, 0, None) == -2
    assert lib.vsr_basicvsr_narrow_get_flows(ctypes.byref(d), ptrs[0], None, None, None) == -2


def test_num_params_does_not_depend_on_the_width():
    from vsrlab_amd import _lib
    lib = _lib.load()
    for mid in (16, 32, 64):
        assert lib.vsr_basicvsr_num_params(ctypes.byref(_lib.BasicVSRDesc(1, 7, 540, 960, mid, 30, 4, 1))) == 316
        assert lib.vsr_basicvsr_num_params(ctypes.byref(_lib.BasicVSRDesc(1, 7, 540, 960, mid, 5, 2, 1))) == 314 - 8 * 25


def test_cleaner_narrow_workspace_query():
    from vsrlab_amd import _lib
    lib = _lib.load()
    for nb in (0, 1):
        q16 = lib.vsr_cleaner_narrow_workspace_bytes(7, 540, 960, 16, 5, 3, 1, nb)
        q32 = lib.vsr_cleaner_narrow_workspace_bytes(7, 540, 960, 32, 5, 3, 1, nb)
        q64 = lib.vsr_cleaner_workspace_bytes(7, 540, 960, 5, 3, 1, nb)
        assert 0 < q16 < q32 < q64, (nb, q16, q32, q64)
    for mid in (8, 24, 48, 64, 128):
        assert lib.vsr_cleaner_narrow_workspace_bytes(7, 540, 960, mid, 5, 3, 1, 1) == 0, mid


def test_narrow_widths_have_no_cpu_fallback_and_other_widths_fail_loudly():
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core.modules.conv import ResidualBlock, ResidualConv
    from vsrlab_amd.core.modules.upsampling import PixelShufflePack
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    x = torch.rand(1, 2, 3, 16, 16)
    for mid in (16, 32):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            BasicVSR(mid, 1)(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ResidualConv(mid)(torch.rand(1, mid, 8, 8))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ResidualBlock(3 + mid, mid, 1)(torch.rand(1, 3 + mid, 8, 8))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            PixelShufflePack(mid, mid, 2)(torch.rand(1, mid, 8, 8))
    # the width check every narrow-capable entry runs names the supported widths
    for mid in (8, 48, 128):
        with pytest.raises(NotImplementedError, match="16, 32 or 64"):
            VF._check_width(mid, "BasicVSR engine")
