"""CPU checks of the local correlation (core/modules/correlation.py, irr/pwc_modules.py compute_cost_volume): the fp64
restatement of tests/correlation_common.py against the reference's recorded results, and the package's argument handling,
workspace query and aliases.  Nothing here needs a GPU."""
import importlib

import pytest
import torch

import correlation_common as CC
from helpers import golden, rel_err


@pytest.fixture(scope="module")
def gold():
    return golden("correlation")


def _check(gold, tag, key, got):
    """a full tensor, or its stored subsample, to 1e-10 of the golden's largest element; the (sum, norm, projection) to 1e-10"""
    if f"{tag}__{key}" in gold:
        assert rel_err(got, gold[f"{tag}__{key}"].reshape(got.shape)) < 1e-10, (tag, key)
    else:
        assert rel_err(got.flatten()[::CC.sub_stride(got.numel())], gold[f"{tag}__sub__{key}"]) < 1e-10, (tag, key)
    stats, want = CC.grad_stats(f"correlation.{tag}.{key}", got), gold[f"{tag}__stats__{key}"]
    assert float(((stats - want).abs() / want.abs().clamp_min(1.0)).max()) < 1e-10, (tag, key, stats, want)


@pytest.mark.parametrize("case", list(CC.CASES))
def test_restatement_equals_the_reference(case, gold):
    shape, patch, stride, padding, _ = CC.CASES[case]
    out, d1, d2 = CC.restate(case)
    assert tuple(out.shape) == CC.out_shape(shape, patch, stride, padding)
    for key, v in (("out", out), ("d_input1", d1), ("d_input2", d2)):
        _check(gold, case, key, v)


def test_cost_volume_restatement_equals_the_reference(gold):
    out, d1, d2 = CC.restate_cost_volume()
    n, _, h, w = CC.CASES[CC.COST_CASE][0]
    assert tuple(out.shape) == (n, (2 * CC.COST_MAX_DISP + 1) ** 2, h, w)
    for key, v in (("out", out), ("d_input1", d1), ("d_input2", d2)):
        _check(gold, "cost", key, v)


def test_output_shapes_for_odd_sizes_and_stride_2():
    assert CC.out_shape((2, 5, 9, 10), (3, 5), 2, (1, 2)) == (2, 3, 5, 6, 7)        # ceil(11 / 2), ceil(14 / 2)
    assert CC.out_shape((1, 7, 10, 9), (7, 3), (2, 1), (2, 0)) == (1, 7, 3, 7, 9)
    assert CC.out_shape((1, 3, 7, 5), 3, 2, 0) == (1, 3, 3, 4, 3)
    x = torch.zeros(1, 3, 7, 5, dtype=torch.float64)
    assert tuple(CC.spatial_correlation_ref(x, x, 3, 2, 0, 1).shape) == (1, 3, 3, 4, 3)
    assert tuple(CC.spatial_correlation_ref(x, x, (5, 3), (1, 2), (2, 1), (1, 1)).shape) == (1, 5, 3, 11, 4)


def test_the_three_refusals_of_the_reference():
    from vsrlab_amd.core.modules.correlation import SpatialCorrelationSampler, iter_spatial_correlation_sample
    x = torch.zeros(1, 4, 6, 6)
    for kw in (dict(kernel_size=3), dict(kernel_size=(1, 3)), dict(dilation=2), dict(dilation=(2, 1)), dict(patch_size=4),
               dict(patch_size=(3, 2))):
        with pytest.raises(NotImplementedError):
            iter_spatial_correlation_sample(x, x, **kw)
        with pytest.raises(NotImplementedError):
            SpatialCorrelationSampler(**kw)(x, x)


UNSUPPORTED = [dict(patch_size=11), dict(patch_size=(3, 11)), dict(patch_size=3, stride=3), dict(patch_size=3, stride=(1, 3)),
               dict(patch_size=3, dilation_patch=3), dict(patch_size=3, padding=2), dict(patch_size=(5, 3), padding=(2, 2)),
               dict(patch_size=1, padding=1)]


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_unsupported_descriptors(kw):
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core.modules.correlation import iter_spatial_correlation_sample
    assert VF.spatial_corr_workspace_bytes((1, 4, 12, 12), **kw) == 0
    x = torch.zeros(1, 4, 12, 12)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        VF.spatial_correlation(x, x, **kw)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        iter_spatial_correlation_sample(x, x, **kw)


def test_library_exports_and_workspace():
    """the entry points live in a library of their own, which exports them and nothing else; the product library's pinned
    symbol set (tests/test_hr_tail_host.py) does not contain them"""
    import os
    import re
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load_spatial_corr()
    names = {"vsr_spatial_corr_workspace_bytes", "vsr_spatial_corr_fwd", "vsr_spatial_corr_bwd"}
    assert set(_lib.SPATIAL_CORR_EXPORTS) == names and not names & set(_lib.EXPORTS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vsrlab_spatial_corr.h")).read()
    assert set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header)) == names
    from test_hr_tail_host import _exported_vsr_symbols          # the dynamic symbol table, read from the ELF file
    assert _exported_vsr_symbols(_lib.SPATIAL_CORR_LIB_PATH) == names
    assert _lib.load().vsr_abi_version() == 4 and not any(hasattr(_lib.load(), n) for n in names)
    # two maps of N H W pixels, channels padded to 8, in the storage type; each rounded up to 256 bytes
    for (shape, patch, stride, padding, dil) in CC.CASES.values():
        n, c, h, w = shape
        elems = n * h * w * ((c + 7) // 8 * 8)
        b32 = VF.spatial_corr_workspace_bytes(shape, patch, stride, padding, dil, _lib.DT_F32)
        b16 = VF.spatial_corr_workspace_bytes(shape, patch, stride, padding, dil, _lib.DT_BF16)
        assert 2 * elems * 4 <= b32 <= 2 * elems * 4 + 512 and 2 * elems * 2 <= b16 <= 2 * elems * 2 + 512
    assert VF.spatial_corr_workspace_bytes((1, 4, 4096, 4096), 9) > 0
    assert VF.spatial_corr_workspace_bytes((1, 4, 4096, 4097), 9) == 0            # H' W' above 2^24
    assert VF.spatial_corr_workspace_bytes((17, 4, 4096, 4096), 9) == 0           # N H' W' above 2^28
    assert VF.spatial_corr_workspace_bytes((1, 4, 4095, 4096), 3, padding=1) == 0  # the padded frame counts
    desc = _lib.SpatialCorrDesc(1, 4, 8, 8, 3, 3, 1, 1, 0, 0, 1, 1, 7, 1.0)        # no such dtype
    assert lib.vsr_spatial_corr_workspace_bytes(desc) == 0 and lib.vsr_spatial_corr_fwd(desc, None, None, None, None, 0, None) == -1
    desc = _lib.SpatialCorrDesc(1, 4, 8, 8, 11, 3, 1, 1, 0, 0, 1, 1, _lib.DT_F32, 1.0)
    assert lib.vsr_spatial_corr_fwd(desc, None, None, None, None, 0, None) == -2   # refused before any pointer is looked at
    assert lib.vsr_spatial_corr_bwd(desc, None, None, None, None, None, None, 0, None) == -2
    desc = _lib.SpatialCorrDesc(1, 4, 8, 8, 3, 3, 1, 1, 0, 0, 1, 1, _lib.DT_F32, 1.0)
    assert lib.vsr_spatial_corr_fwd(desc, None, None, None, None, 0, None) == -1   # null pointers


def test_validation_and_cpu_tensors():
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core.modules.correlation import SpatialCorrelationSampler, iter_spatial_correlation_sample
    from vsrlab_amd.optical_flow.models.irr.pwc_modules import compute_cost_volume
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError):
        VF.spatial_correlation(x, torch.zeros(1, 4, 8, 9), 3)
    with pytest.raises(ValueError):
        VF.spatial_correlation(x, x, 3, stride=0)
    with pytest.raises(ValueError):
        VF.spatial_correlation(x, x, 3, padding=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VF.spatial_correlation(x, x, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iter_spatial_correlation_sample(x, x, patch_size=(3, 5), stride=2, padding=(1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SpatialCorrelationSampler(patch_size=9)(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_cost_volume(x, x, {"max_disp": 4})
    m = SpatialCorrelationSampler()
    assert (m.kernel_size, m.patch_size, m.stride, m.padding, m.dilation, m.dilation_patch) == (1, 1, 1, 0, 1, 1)


def test_aliases_resolve():
    from vsrlab_amd.compat import install_as_vsrlab
    install_as_vsrlab(force=True)
    m = importlib.import_module("vsrlab.core.modules.correlation")
    assert hasattr(m, "SpatialCorrelationSampler") and hasattr(m, "iter_spatial_correlation_sample")
    assert hasattr(importlib.import_module("vsrlab.optical_flow.models.irr.pwc_modules"), "compute_cost_volume")
    assert importlib.import_module("vsrlab.optical_flow.models.irr") is importlib.import_module("vsrlab_amd.optical_flow.models.irr")
