"""CPU-side checks of the deformable-convolution surface: dotted paths, state_dict schema recorded from the reference classes
(tests/golden/deform_conv.npz), initialisation, constructor / shape validation, exported symbols, and the fp64 restatement
(tests/deform_common.py) against the golden outputs, which guards the fixture and the helper against each other."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import deform_common as DC
from helpers import GOLDEN, rel_err


def _z():
    return np.load(os.path.join(GOLDEN, "deform_conv.npz"), allow_pickle=False)


def _schema(z, tag):
    return [(str(k), tuple(int(i) for i in str(s).split(";"))) for k, s in zip(z[tag + "__keys"], z[tag + "__shapes"])]


def _sd_schema(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_reference_dotted_paths_resolve():
    from vsrlab_amd.compat import install_as_vsrlab
    install_as_vsrlab(force=True)
    mod = importlib.import_module("vsrlab.vsr.models.VRT.modules.deform_conv")
    for name in ("ModulatedDeformConv", "ModulatedDeformConvPack", "DCNv2PackFlowGuided"):
        assert hasattr(mod, name)
    conv = importlib.import_module("vsrlab.core.modules.conv")
    assert hasattr(conv, "DeformConv") and hasattr(conv, "DeformBlock")


def test_state_dict_schema_equals_the_reference():
    from vsrlab_amd.core.modules.conv import DeformBlock
    from vsrlab_amd.vsr.models.VRT.modules import deform_conv as M
    z = _z()
    for tag, c in DC.DCN_CASES.items():
        m = M.DCNv2PackFlowGuided(c["C"], c["C"], 3, padding=1, deformable_groups=c["dg"], max_residue_magnitude=10, pa_frames=2)
        assert _sd_schema(m) == _schema(z, tag)
    assert _sd_schema(M.ModulatedDeformConv(32, 32, 3, padding=1, deformable_groups=4)) == _schema(z, "mdc")
    assert _sd_schema(M.ModulatedDeformConvPack(32, 32, 3, padding=1, deformable_groups=4)) == _schema(z, "mdcp")
    c = DC.BLOCK_CASE
    assert _sd_schema(DeformBlock(c["cin"], c["mid"], c["blocks"])) == _schema(z, "blk")


def test_initialisation():
    from vsrlab_amd.core.modules.conv import DeformConv
    from vsrlab_amd.vsr.models.VRT.modules import deform_conv as M
    m = M.DCNv2PackFlowGuided(32, 32, 3, padding=1, deformable_groups=4, max_residue_magnitude=7, pa_frames=2)
    assert m.max_residue_magnitude == 7 and m.pa_frames == 2
    assert float(m.conv_offset[-1].weight.abs().max()) == 0 and float(m.conv_offset[-1].bias.abs().max()) == 0
    assert float(m.conv_offset[0].weight.abs().max()) > 0
    bound = 1 / math.sqrt(32 * 9)
    assert 0.9 * bound < float(m.weight.abs().max()) <= bound and float(m.bias.abs().max()) == 0
    p = M.ModulatedDeformConvPack(32, 32, 3, padding=1, deformable_groups=4)
    assert float(p.conv_offset.weight.abs().max()) == 0 and tuple(p.conv_offset.weight.shape) == (4 * 27, 32, 3, 3)
    d = DeformConv(2, 64, 64, 3, padding=1)
    assert float(d.conv_offset.weight.abs().max()) == 0 and tuple(d.conv_offset.weight.shape) == (36, 64, 3, 3)
    kb = math.sqrt(6 / ((1 + 5) * 64 * 9))          # kaiming_uniform(a = sqrt 5): sqrt(6 / ((1 + a^2) fan_in))
    assert 0.9 * kb < float(d.weight.abs().max()) <= kb and 0 < float(d.bias.abs().max()) <= 1 / math.sqrt(64 * 9)


def test_constructor_validation():
    from vsrlab_amd.core.modules.conv import DeformConv
    from vsrlab_amd.vsr.models.VRT.modules import deform_conv as M
    with pytest.raises(ValueError):                  # the reference's vrt.yaml: embed_dims 120 with deformable_groups 16
        M.DCNv2PackFlowGuided(120, 120, 3, padding=1, deformable_groups=16)
    with pytest.raises(NotImplementedError):
        M.DCNv2PackFlowGuided(32, 32, 3, stride=2, padding=1, deformable_groups=4)
    with pytest.raises(NotImplementedError):
        DeformConv(1, 64, 64, 3, stride=2, padding=1)
    with pytest.raises(ValueError):
        DeformConv(5, 64, 64, 3, padding=1)


def test_functional_shape_validation():
    from vsrlab_amd import functional as VF
    x, w = torch.zeros(1, 32, 6, 6), torch.zeros(32, 32, 3, 3)
    with pytest.raises(NotImplementedError):
        VF.deform_conv2d(x, torch.zeros(1, 18, 6, 6), w, stride=2)
    with pytest.raises(ValueError):
        VF.deform_conv2d(x, torch.zeros(1, 18 * 5, 6, 6), w)         # 5 groups do not divide 32
    with pytest.raises(ValueError):
        VF.deform_conv2d(x, torch.zeros(1, 18, 6, 6), w, mask=torch.zeros(1, 18, 6, 6))
    with pytest.raises(ValueError):
        VF.flow_guided_deform_conv(x, torch.zeros(1, 27, 6, 6), torch.zeros(1, 2, 5, 6), w, None, 10)
    with pytest.raises(RuntimeError):                # no CPU fallback
        VF.deform_conv2d(x, torch.zeros(1, 18, 6, 6), w)


def test_library_exports_and_workspace():
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load()
    for name in ("vsr_deform_conv_workspace_bytes", "vsr_deform_conv_fwd", "vsr_deform_conv_bwd", "vsr_deform_offset_mask"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.vsr_abi_version() == 4
    fwd = VF.deform_conv_workspace_bytes((2, 120, 20, 28), 120, 8, _lib.DT_BF16, False)
    bwd = VF.deform_conv_workspace_bytes((2, 120, 20, 28), 120, 8, _lib.DT_BF16, True)
    assert 0 < fwd < bwd
    assert VF.deform_conv_workspace_bytes((1, 256, 8, 8), 64, 1) == 0          # Cin > 192
    assert VF.deform_conv_workspace_bytes((1, 120, 8, 8), 64, 16) == 0         # 16 does not divide 120
    assert VF.deform_conv_workspace_bytes((1, 180, 8, 8), 64, 18) == 0         # 18 groups of 10, padded to 16, exceed 192
    for cpg_case in ((32, 4), (120, 12), (120, 8), (64, 1), (180, 12)):
        assert VF.deform_conv_workspace_bytes((1, cpg_case[0], 8, 8), cpg_case[0], cpg_case[1]) > 0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_the_golden(tag):
    """our module's wiring evaluated in fp64 with the restatement == the reference module's output"""
    import torch.nn.functional as F
    z = _z()
    c = DC.DCN_CASES[tag]
    sd = DC.dcn_state_dict({k: torch.empty(s) for k, s in _schema(z, tag)}, tag)
    x, warped, cur, flow, _ = DC.dcn_inputs(tag)
    h = torch.cat([warped, cur, flow], dim=1)
    for i in (0, 2, 4, 6):
        h = F.conv2d(h, sd[f"conv_offset.{i}.weight"], sd[f"conv_offset.{i}.bias"], padding=1)
        if i < 6:
            h = F.leaky_relu(h, 0.1)
    y = DC.flow_guided_deform_conv_ref(x, h, flow, sd["weight"], sd["bias"], 10)
    if y.numel() <= DC.BIG:
        assert rel_err(y, torch.from_numpy(z[tag + "__y"])) < 1e-12
    else:
        assert rel_err(y.flatten()[::DC.sub_stride(y.numel())], torch.from_numpy(z[tag + "__sub__y"])) < 1e-12
    assert abs(float(y.norm()) / float(z[tag + "__stats__y"][1]) - 1) < 1e-12


def test_restatement_matches_grid_sample():
    """independent formulation: grid_sample(bilinear, zeros, align_corners=True) in pixel coordinates"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    N, C, H, W, dg = 1, 8, 9, 11, 2
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    off = torch.randn(N, 18 * dg, H, W, generator=g, dtype=torch.float64) * 4
    mask = torch.rand(N, 9 * dg, H, W, generator=g, dtype=torch.float64)
    col = DC.deform_columns(x, off, mask).reshape(N, dg, C // dg, 9, H, W)
    py, px = DC.sample_positions(off, H, W)
    for gi in range(dg):
        for k in range(9):
            grid = torch.stack([px[:, gi, k] * 2 / (W - 1) - 1, py[:, gi, k] * 2 / (H - 1) - 1], dim=-1)
            ref = F.grid_sample(x[:, gi * (C // dg):(gi + 1) * (C // dg)], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            ref = ref * mask[:, gi * 9 + k].unsqueeze(1)
            assert float((col[:, gi, :, k] - ref).abs().max()) < 1e-12
